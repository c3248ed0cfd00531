"""BGZF files written block by block in Python (zlib and struct only), for the
block-checksum tests: a file from a list of payloads, each block level-1
DEFLATE or stored (BTYPE 0: its payload bytes stand in the file as they are),
every block's file offset, the file offset of a stored block's payload bytes,
a flipped bit in a block's stored CRC-32, the EOF marker dropped; the length
grid; and the "silent damage" BAM, a generated BAM whose one damaged byte
still inflates to the right length."""
import os
import random
import struct
import zlib

from _handmade import _header_len, _inflate, _records, inflated
from _util import CASES, synth

EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

# payload lengths: an empty block mid-file, one byte, around the 16-byte chunk,
# the 64-byte line, one lane's stride (1008 + 16), two and four strides, and
# the sizes BGZF writers fill blocks to
GRID = (0, 1, 15, 16, 17, 63, 64, 65, 1007, 1008, 1023, 1024, 1025, 2047, 2048, 2049, 4093, 65279, 65280)
FILLS = ("random", "zeros", "ones")


def block(payload, stored=False):
    """One BGZF block; a stored one is a single final BTYPE-0 block: 5 bytes, then the payload."""
    if stored:  # (written out: zlib's level 0 splits a payload of 32 KB or more into two)
        z = b"\x01" + struct.pack("<HH", len(payload), len(payload) ^ 0xffff) + payload
        assert zlib.decompress(z, -15) == payload
    else:
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        z = c.compress(payload) + c.flush()
    assert len(z) + 26 <= 65536, (len(payload), len(z))
    return (struct.pack("<4BI2BH2B2H", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(z) + 25) + z +
            struct.pack("<II", zlib.crc32(payload), len(payload)))


def write_bgzf(path, payloads, stored=(), eof=True):
    """The payloads as one BGZF file (blocks whose index is in `stored` are
    stored blocks), the EOF marker last.  Returns one dict per payload: `off`
    the block's file offset, `end` the offset after it, `n` its payload length,
    `data` the file offset of its payload's first byte (stored blocks) or None."""
    info, parts, o = [], [], 0
    for i, p in enumerate(payloads):
        st = i in stored
        b = block(p, st)
        one = st and len(p) > 0 and len(b) == 18 + 5 + len(p) + 8 and b[23:23 + len(p)] == p  # (one BTYPE-0 block)
        info.append({"off": o, "end": o + len(b), "n": len(p), "data": o + 18 + 5 if one else None})
        parts.append(b)
        o += len(b)
    if eof:
        b = block(b"")
        assert b == EOF_MARKER
        parts.append(b)
    with open(path, "wb") as f:
        f.write(b"".join(parts))
    return info


def flip_crc_bit(path, blk, bit=0):
    """One bit of the block's stored CRC-32 (the 4 bytes before ISIZE) flipped."""
    with open(path, "r+b") as f:
        f.seek(blk["end"] - 8 + bit // 8)
        v = f.read(1)[0]
        f.seek(blk["end"] - 8 + bit // 8)
        f.write(bytes([v ^ (1 << (bit % 8))]))


def drop_eof(path):
    d = open(path, "rb").read()
    assert d.endswith(EOF_MARKER)
    with open(path, "wb") as f:
        f.write(d[:-len(EOF_MARKER)])


def fill_bytes(fill, n, rng):
    return rng.randbytes(n) if fill == "random" else (b"\x00" if fill == "zeros" else b"\xff") * n


def grid_payloads():
    """The grid's lengths with every fill, ordered so that the blocks' offsets
    in the inflated stream cover all 16 residues mod 16 (asserted): the odd
    lengths come between the even ones."""
    rng = random.Random(20260101)
    lens = []
    for k, fill in enumerate(FILLS):
        order = list(GRID[k:]) + list(GRID[:k])  # (a rotation per fill: other start offsets)
        lens += [(n, fill) for n in order]
    # pad blocks of 1..15 bytes shift the stream through every residue
    for r in range(1, 16):
        lens.append((r, "random"))
        lens.append((65280 if r % 3 == 0 else 4093, "random"))  # (and enough bytes for more than ten 64 KB pieces)
    payloads = [fill_bytes(f, n, rng) for n, f in lens]
    offs, o = [], 0
    for p in payloads:
        offs.append(o)
        o += len(p)
    assert {x % 16 for x, p in zip(offs, payloads) if len(p) >= 1024} == set(range(16))
    assert {x % 16 for x in offs} == set(range(16))
    return payloads


_cache = {}


def grid_file(datadir):
    """{"path", "info", "payloads"}: the grid as one BGZF file (a few hundred
    KB compressed, every fifth block stored), made once."""
    if "grid" not in _cache:
        payloads = grid_payloads()
        path = os.path.join(str(datadir), "crc_grid.bgzf")
        info = write_bgzf(path, payloads, stored=set(range(0, len(payloads), 5)))
        _cache["grid"] = {"path": path, "info": info, "payloads": payloads}
    return _cache["grid"]


def copy_with(src, dst, edit):
    """src copied to dst, then edit(dst)."""
    with open(src, "rb") as f, open(dst, "wb") as g:
        g.write(f.read())
    edit(dst)
    return dst


PIECE = 60000  # the silent-damage BAM's payload bytes per block


def silent_damage(datadir):
    """three_chr's stream written again in blocks of 60000 bytes, the block
    that holds one chosen record's quality bytes a stored block, indexed, and
    one quality byte flipped in the file: {"bam", "good" (the same file before
    the flip), "fa", "block_off" (the damaged block's file offset), "blocks",
    "stream", "u_off" (the byte's offset in the inflated stream)}.  Made once."""
    if "sd" in _cache:
        return _cache["sd"]
    import grom_amd
    _, fa = synth(datadir, "three_chr", CASES["three_chr"])
    stream = inflated(datadir, "three_chr", CASES["three_chr"])
    h, _ = _header_len(stream)
    recs = [r for r in _records(stream, h) if r[2] == 1]
    o, n, _, _ = recs[len(recs) // 2]  # a record in the middle of the second chromosome
    l_qname, = struct.unpack_from("<B", stream, o + 12)
    n_cig, = struct.unpack_from("<H", stream, o + 16)
    l_seq, = struct.unpack_from("<i", stream, o + 20)
    assert l_seq > 8
    u_off = o + 36 + l_qname + 4 * n_cig + (l_seq + 1) // 2 + 5
    assert u_off < o + n
    payloads = [stream[k:k + PIECE] for k in range(0, len(stream), PIECE)]
    b = u_off // PIECE
    good = os.path.join(str(datadir), "crc_good.bam")
    info = write_bgzf(good, payloads, stored={b})
    prev = grom_amd.verify_bgzf_crc(False)
    try:
        assert grom_amd.lib().grom_bai_build(good.encode()) == 0
    finally:
        grom_amd.verify_bgzf_crc(prev)
    bam = os.path.join(str(datadir), "crc_damaged.bam")
    assert info[b]["data"] is not None
    at = info[b]["data"] + (u_off - b * PIECE)

    def flip(path):
        with open(path, "r+b") as f:
            f.seek(at)
            v = f.read(1)[0]
            assert v == stream[u_off]
            f.seek(at)
            f.write(bytes([v ^ 1]))
    copy_with(good, bam, flip)
    copy_with(good + ".bai", bam + ".bai", lambda p: None)
    _cache["sd"] = {"bam": bam, "good": good, "fa": fa, "block_off": info[b]["off"], "block": info[b], "blocks": len(info) + 1,
                    "stream": stream, "u_off": u_off, "info": info}
    return _cache["sd"]


def prove_silent(sd):
    """The damaged file still inflates to the same lengths, exactly one byte
    differs, and the damaged block's CRC-32 is no longer its trailer's."""
    got = _inflate(sd["bam"])
    stream = sd["stream"]
    assert len(got) == len(stream)
    diff = [i for i in range(sd["u_off"] - 64, sd["u_off"] + 64) if got[i] != stream[i]]
    assert diff == [sd["u_off"]] and got[:sd["u_off"] - 64] == stream[:sd["u_off"] - 64] and \
        got[sd["u_off"] + 64:] == stream[sd["u_off"] + 64:]
    d = open(sd["bam"], "rb").read()
    blk = sd["block"]
    k = sd["u_off"] // PIECE
    stored_crc, isize = struct.unpack_from("<II", d, blk["end"] - 8)
    payload = got[k * PIECE:(k + 1) * PIECE]
    assert isize == len(payload) and zlib.crc32(payload) != stored_crc
    assert zlib.crc32(stream[k * PIECE:(k + 1) * PIECE]) == stored_crc
