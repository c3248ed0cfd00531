"""The hand-made VCF texts of the sorting, indexing VCF writer's tests (host
twin and device), and the checks every output must pass against Python's own
sort and the independent tabix reader (_tabix.py)."""
import gzip
import os
import random

import _bgzf_write as W
import _tabix as T

HDR = b"##fileformat=VCFv4.2\n##source=grid\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\n"
LIMIT = 1 << 29


def row(chrom, pos, ref="A", info=".", pad=0, tag=""):
    tail = ("x" * pad) if pad else "0/1"
    return f"{chrom}\t{pos}\t{tag}\t{ref}\tG\t.\t.\t{info}\tGT\t{tail}\n".encode()


def _shuffled(rng, rows):
    rows = list(rows)
    rng.shuffle(rows)
    return rows


def grid():
    """[(name, text)], the same list every time."""
    rng = random.Random(20261021)
    out = []
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 4097):
        rows = [row("c1" if k % 3 else "c2", rng.randrange(1, 3_000_000), tag=f"r{k}") for k in range(n)]
        out.append((f"rows{n}", HDR + b"".join(rows)))
    out.append(("no_header", b"".join(row("c1", p) for p in (5, 3, 9))))
    out.append(("one_pos", HDR + b"".join(row("c1", 777, tag=f"k{k}") for k in range(300))))
    srt = [row("c1", 10 + 7 * k, tag=f"s{k}") for k in range(1500)] + [row("c2", 5 + k, tag=f"t{k}") for k in range(700)]
    out.append(("sorted", HDR + b"".join(srt)))
    out.append(("reverse", HDR + b"".join(reversed(srt))))
    out.append(("contigs300", HDR + b"".join(row(f"ctg{k % 300}", 1 + (k * 7919) % 100_000, tag=f"i{k}") for k in range(1200))))
    out.append(("low_bits", HDR + b"".join(row("c1", 4096 + v) for v in _shuffled(rng, range(256)))))
    out.append(("high_bits", HDR + b"".join(row("c1", (v << 24) + 5) for v in _shuffled(rng, range(1, 32)))))
    out.append(("pos0", HDR + row("c1", 7) + row("c1", 0) + row("c1", 1)))
    out.append(("last_pos", HDR + row("c1", LIMIT - 1) + row("c1", 12)))
    lv = []
    for s in (14, 17, 20, 23, 26):
        lv.append(row("c1", (1 << s) - 10, ref=".", info=f"END={(1 << s) + 10}"))
        lv.append(row("c1", (3 << s) - 1, ref=".", info=f"SVTYPE=DEL;END={(3 << s) + 1}"))
    out.append(("levels", HDR + b"".join(_shuffled(rng, lv))))
    out.append(("end_keys", HDR + row("c1", 900, info="END=70000") + row("c1", 800, info="DP=3;END=50000;AF=1") +
                row("c1", 700, info="XEND=5") + row("c1", 600, info="END") + row("c1", 500, info="A=1;END") +
                row("c1", 400, info="END=399") + row("c1", 300, info="END=12") + row("c1", 200, ref=".") +
                row("c1", 100, ref="ACGTACGT") + row("c1", 50, info="END=") + row("c1", 40, info="MEND=9;END=90000")))
    out.append(("long_row", HDR + row("c1", 50) + row("c1", 20, pad=70_000) + row("c1", 30) + row("c2", 5, pad=66_000)))
    # rows whose starts cover all 16 residues mod 16, in the input and in the sorted stream
    rr = [row("c1", 5000 - 3 * k, pad=1 + (k * 7) % 19, tag=f"a{k}") for k in range(200)]
    res_in, res_out, o = set(), set(), len(HDR)
    for r in rr:
        res_in.add(o % 16)
        o += len(r)
    o = len(HDR)
    for r in reversed(rr):
        res_out.add(o % 16)
        o += len(r)
    assert res_in == set(range(16)) and res_out == set(range(16)), (sorted(res_in), sorted(res_out))
    out.append(("residues", HDR + b"".join(rr)))
    # a row that ends exactly at a multiple of 65280 in the sorted stream
    body = [row("c1", 100 + k, pad=50, tag=f"b{k}") for k in range(1200)]
    exact = row("c1", 90, pad=1)  # the lowest POS: the first sorted row, which ends where the first block ends
    exact = row("c1", 90, pad=1 + W.MAX - len(HDR) - len(exact))
    assert len(HDR) + len(exact) == W.MAX
    body = _shuffled(rng, body)
    out.append(("block_end", HDR + b"".join(body[:600]) + exact + b"".join(body[600:])))
    return out


REFUSED = [
    ("no_newline", HDR + row("c1", 5) + row("c1", 3)[:-1], "the last line does not end in a newline"),
    ("hash_after_row", HDR + row("c1", 5) + b"##late\n" + row("c1", 3), "line 5: a '#' line after the first row"),
    ("seven_columns", HDR + row("c1", 5) + b"c1\t4\t.\tA\tG\t.\t.\n", "line 5: fewer than 8 columns"),
    ("pos_12x", HDR + row("c1", "12x"), "line 4: POS is not a decimal number"),
    ("past_limit", HDR + row("c1", 5) + row("c1", LIMIT, ref="AC"), "line 5: the row ends past 2^29: the .tbi index is limited to 512 Mb"),
]


def regions(data):
    """[(name, beg, end)] asked of every output: each row's own span, each
    symbolic allele's span, every contig whole, an empty stretch and one past
    the last row."""
    out = [(s[0], s[2], s[3]) for s in data.spans]
    for nm in data.names:
        out.append((nm, 0, 1 << 29))
    if data.spans:
        nm = data.names[0]
        last = max(s[3] for s in data.spans if s[0] == nm)
        out.append((nm, last + 50_000, last + 60_000))  # past the last row
        out.append((nm, last, last))                    # nothing
        out.append((b"no_such_contig", 0, 1000))
        ends = sorted(s[3] for s in data.spans if s[0] == nm)
        begs = sorted(s[2] for s in data.spans if s[0] == nm)
        for e in ends:  # a stretch no row covers, when there is one
            nxt = [b for b in begs if b > e]
            if nxt and nxt[0] - e > 2 and not any(s[2] < nxt[0] - 1 and s[3] > e + 1 for s in data.spans if s[0] == nm):
                out.append((nm, e + 1, nxt[0] - 1))
                break
    return out


def check_output(text, path, stats=None, full_queries=True):
    """OUT.gz, OUT.gz.tbi and OUT.gz.gzi against the input text."""
    hdr, rows, names = T.sorted_text(text)
    got = gzip.decompress(open(path, "rb").read())
    assert got == hdr + b"".join(rows), "not the header followed by the stably sorted rows"
    assert sorted(got.splitlines(True)) == sorted(text.splitlines(True))
    raw = open(path, "rb").read()
    assert raw.endswith(W.EOF_MARKER)
    blocks = W.walk(raw)
    assert all(int.from_bytes(b[-4:], "little") == W.MAX for _, _, b in blocks[:-2])
    assert W.read_gzi(path + ".gzi") == [(c, u) for c, u, _ in blocks[1:-1]]
    tbi, data = T.parse_tbi(path + ".tbi"), T.Data(path)
    assert data.rows == rows and tbi["names"] == names
    if not rows:
        assert tbi["n_ref"] == 0
    T.check_structure(tbi, data)
    regs = regions(data)
    if not full_queries and len(regs) > 400:
        regs = regs[::max(1, len(regs) // 300)] + regs[-8:]
    for nm, b, e in regs:
        assert T.query(tbi, data, nm, b, e) == T.brute(data, nm, b, e), (nm, b, e)
    if stats is not None:
        assert stats["rows"] == len(rows) and stats["contigs"] == len(names), stats
        assert stats["header_lines"] == len(hdr.splitlines()), stats
    return tbi, data


def files(path):
    return tuple(open(path + s, "rb").read() for s in ("", ".tbi", ".gzi"))


def leftovers(d):
    return sorted(os.listdir(d))
