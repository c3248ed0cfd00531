"""The payload grid of the BGZF writer's tests (host twin and device): the
lengths and contents at which the compressor takes another path, laid out back
to back so that the payloads' starts cover all 16 residues mod 16, and the
checks every block must pass against Python's zlib."""
import os
import random
import zlib

from _util import GOLDEN_VCF, TILAPIA_FA

MAX = 65280
LENGTHS = (0, 1, 2, 3, 4, 257, 258, 259, 260, 32767, 32768, 32769, 65279, 65280)
PERIODS = (1, 2, 3, 4, 32767, 32768, 32769)
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _copies(rng):
    """A copy of every length 3..258, and copies at distances that hit all 30
    distance codes, 32768 among them: random stretches repeated exactly, the
    byte after each copy different from the source's."""
    s = rng.randbytes(259)
    out = bytearray(s)
    for n in range(3, 259):  # s[:n], then a byte that is not s[n]: a copy of exactly n bytes
        out += s[:n] + bytes([s[n] ^ 0xff])
    assert len(out) > 32768 + 8
    # the distance codes' first distances (RFC 1951 3.2.5) and the last one
    firsts = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
              6145, 8193, 12289, 16385, 24577, 32768]
    assert len(firsts) == 31
    for d in firsts:
        src = len(out) - d
        seg = bytes(out[src:src + 8]) if d >= 8 else (bytes(out[src:]) * 8)[:8]
        out += seg + rng.randbytes(3)
    assert len(out) <= MAX
    return bytes(out)


def _fibonacci(rng):
    """Byte k occurs F(k + 1) times, k < 22 (46,367 bytes), shuffled: an
    unlimited Huffman tree over it is 21 deep."""
    f, out = [1, 1], bytearray()
    while len(f) < 22:
        f.append(f[-1] + f[-2])
    for k, c in enumerate(f):
        out += bytes([65 + k]) * c
    assert len(out) == 46367
    lst = list(out)
    rng.shuffle(lst)
    return bytes(lst)


def _file_cuts(path):
    d = open(path, "rb").read()[:200000]
    return [d[i:i + MAX] for i in range(0, len(d), MAX)]


def payloads():
    """[(name, bytes)], the same list every time."""
    rng = random.Random(20261021)
    out = []
    for n in LENGTHS:
        out.append((f"random{n}", rng.randbytes(n)))
        out.append((f"zeros{n}", bytes(n)))
        out.append((f"ff{n}", b"\xff" * n))
    out.append(("letter1", b"A"))
    out.append(("letter2", b"AA"))
    for p in PERIODS:
        base = rng.randbytes(p)
        out.append((f"period{p}", (base * (MAX // p + 1))[:MAX]))
    out.append(("copies", _copies(rng)))
    out.append(("fibonacci", _fibonacci(rng)))
    out += [(f"vcf{i}", b) for i, b in enumerate(_file_cuts(GOLDEN_VCF))]
    out += [(f"fasta{i}", b) for i, b in enumerate(_file_cuts(TILAPIA_FA))]
    # back to back from offset 0 the starts must cover every residue mod 16: odd one-byte spacers do it
    res, o, laid = set(), 0, []
    for k, (name, b) in enumerate(out):
        laid.append((name, b))
        res.add(o % 16)
        o += len(b)
        if k % 3 == 2:
            laid.append((f"spacer{k}", bytes([k & 255]) * (1 + k % 5)))
            res.add(o % 16)
            o += 1 + k % 5
    assert res == set(range(16)), sorted(res)
    return laid


def check_block(name, payload, blk):
    """One BGZF block against its payload: header, BSIZE, ISIZE, CRC-32,
    zlib's decoder, the size bound.  Returns BTYPE."""
    assert blk[:16] == bytes.fromhex("1f8b08040000000000ff060042430200"), (name, blk[:18].hex())
    assert int.from_bytes(blk[16:18], "little") == len(blk) - 1, name
    assert int.from_bytes(blk[-4:], "little") == len(payload), name
    assert int.from_bytes(blk[-8:-4], "little") == zlib.crc32(payload), name
    d = zlib.decompressobj(-15)
    got = d.decompress(blk[18:-8])
    assert got == payload and d.eof and d.unused_data == b"", name
    assert len(blk) <= len(payload) + 31, (name, len(blk))
    assert blk[18] & 1 == 1, name  # one final block
    return (blk[18] >> 1) & 3


def walk(data):
    """[(compressed offset, uncompressed offset, block bytes)] of a BGZF file."""
    out, o, u = [], 0, 0
    while o < len(data):
        n = int.from_bytes(data[o + 16:o + 18], "little") + 1
        out.append((o, u, data[o:o + n]))
        u += int.from_bytes(data[o + n - 4:o + n], "little")
        o += n
    assert o == len(data)
    return out


def read_gzi(path):
    d = open(path, "rb").read()
    n = int.from_bytes(d[:8], "little")
    assert len(d) == 8 + 16 * n, (len(d), n)
    return [(int.from_bytes(d[8 + 16 * i:16 + 16 * i], "little"), int.from_bytes(d[16 + 16 * i:24 + 16 * i], "little"))
            for i in range(n)]


def z1_size(data):
    """The sum over the 65280-byte payloads of zlib level 1's raw DEFLATE size + 26."""
    t = 0
    for i in range(0, len(data), MAX):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        t += len(c.compress(data[i:i + MAX]) + c.flush()) + 26
    return t


def tmp_env(monkeypatch, piece_kb):
    if piece_kb is None:
        monkeypatch.delenv("GROM_BGZF_PIECE_KB", raising=False)
    else:
        monkeypatch.setenv("GROM_BGZF_PIECE_KB", str(piece_kb))
    return os.environ.get("GROM_BGZF_PIECE_KB")
