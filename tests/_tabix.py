"""An independent reader of bgzipped, tabix-indexed VCF, written from the
tabix specification (the .tbi layout, the UCSC binning scheme with min shift
14 and 5 levels, BGZF virtual offsets): the yardstick of the sorting VCF
writer's tests, never the project's own reader.  Python's gzip inflates the
.tbi, _bgzf_write.walk and zlib inflate the data file's blocks."""
import bisect
import gzip
import struct
import zlib

import numpy as np

import _bgzf_write as W

PSEUDO_BIN = 37450


def row_span(line):
    """(CHROM, POS, beg0, end0) of a VCF row by the writer's documented rule."""
    f = line.rstrip(b"\n").split(b"\t")
    pos = int(f[1])
    beg0 = max(pos - 1, 0)
    end0 = beg0 + len(f[3])
    for kv in f[7].split(b";"):
        if kv.startswith(b"END="):
            digits = kv[4:]
            k = 0
            while k < len(digits) and digits[k:k + 1].isdigit():
                k += 1
            v = int(digits[:k]) if k else 0
            if v > beg0:
                end0 = v
            break
    if end0 <= beg0:
        end0 = beg0 + 1
    return f[0], pos, beg0, end0


def sorted_text(text):
    """(header bytes, rows stably sorted by (contig in order of first appearance, POS))."""
    lines = text.splitlines(True)
    h = 0
    while h < len(lines) and lines[h].startswith(b"#"):
        h += 1
    order = {}
    for l in lines[h:]:
        order.setdefault(l.split(b"\t", 1)[0], len(order))
    rows = sorted(lines[h:], key=lambda l: (order[l.split(b"\t", 1)[0]], int(l.split(b"\t", 2)[1])))
    return b"".join(lines[:h]), rows, list(order)


def parse_tbi(path):
    raw = open(path, "rb").read()
    assert raw.endswith(W.EOF_MARKER), "the .tbi does not end with the BGZF EOF marker"
    d = gzip.decompress(raw)
    assert d[:4] == b"TBI\1"
    n_ref, fmt, col_seq, col_beg, col_end, meta, skip, l_nm = struct.unpack_from("<8i", d, 4)
    o = 36
    names = d[o:o + l_nm].split(b"\0")[:-1] if l_nm else []
    assert len(names) == n_ref and (l_nm == 0 or d[o + l_nm - 1] == 0)
    o += l_nm
    refs = []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<i", d, o)
        o += 4
        bins, pseudo = {}, None
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", d, o)
            o += 8
            chunks = [struct.unpack_from("<QQ", d, o + 16 * k) for k in range(n_chunk)]
            o += 16 * n_chunk
            if b == PSEUDO_BIN:
                assert n_chunk == 2 and pseudo is None
                pseudo = chunks[0] + chunks[1]  # offset span, mapped, unmapped
            else:
                assert b not in bins and b < PSEUDO_BIN
                bins[b] = chunks
        (n_intv,) = struct.unpack_from("<i", d, o)
        o += 4
        lin = list(struct.unpack_from(f"<{n_intv}Q", d, o))
        o += 8 * n_intv
        refs.append({"bins": bins, "pseudo": pseudo, "lin": lin})
    (n_no_coor,) = struct.unpack_from("<Q", d, o)
    assert o + 8 == len(d), (o, len(d))
    return {"n_ref": n_ref, "format": fmt, "col_seq": col_seq, "col_beg": col_beg, "col_end": col_end, "meta": meta,
            "skip": skip, "names": names, "refs": refs, "n_no_coor": n_no_coor}


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


class Data:
    """The rows of a BGZF VCF with their virtual offsets, read block by block."""

    def __init__(self, path):
        raw = open(path, "rb").read()
        self.blocks = []  # (compressed offset, payload)
        for coff, _, blk in W.walk(raw):
            z = zlib.decompressobj(-15)
            payload = z.decompress(blk[18:-8])
            assert z.eof and int.from_bytes(blk[-4:], "little") == len(payload)
            self.blocks.append((coff, payload))
        assert self.blocks and self.blocks[-1][1] == b"", "no EOF block"
        self.text = b"".join(p for _, p in self.blocks)
        # virtual offset of every uncompressed byte position that starts a line (and of the end)
        starts, u = [], 0
        self._ubase = []
        for coff, p in self.blocks:
            self._ubase.append(u)
            u += len(p)
        lines = self.text.splitlines(True)
        assert not lines or lines[-1].endswith(b"\n")
        o = 0
        self.header, self.rows = [], []
        vs = []
        for l in lines:
            if l.startswith(b"#") and not self.rows:
                self.header.append(l)
            else:
                self.rows.append(l)
                vs.append(o)
            o += len(l)
        self.vbeg = [self.voff(x) for x in vs]
        self.vend = self.vbeg[1:] + [self.voff(len(self.text))]
        spans = [row_span(l) for l in self.rows]
        self.names = []
        for s in spans:
            if not self.names or self.names[-1] != s[0]:
                self.names.append(s[0])
        ids = {nm: i for i, nm in enumerate(self.names)}
        self.cid = np.array([ids[s[0]] for s in spans], dtype=np.int64)
        self.beg0 = np.array([s[2] for s in spans], dtype=np.int64)
        self.end0 = np.array([s[3] for s in spans], dtype=np.int64)
        self.spans = spans

    def voff(self, u):
        """The virtual offset of uncompressed position u: a position at a
        block's end belongs to the next block's start."""
        k = bisect.bisect_right(self._ubase, u) - 1
        while k + 1 < len(self.blocks) and u - self._ubase[k] >= len(self.blocks[k][1]):
            k += 1
        return (self.blocks[k][0] << 16) | (u - self._ubase[k])


def query(tbi, data, name, beg, end):
    """The standard tabix query of [beg, end) (0-based): the candidate bins,
    the chunks whose end is above the linear offset of beg >> 14, the rows read
    through the chunks, those that overlap kept.  Returns row indices."""
    if name not in tbi["names"]:
        return []
    t = tbi["names"].index(name)
    ref = tbi["refs"][t]
    lin = ref["lin"]
    w = beg >> 14
    min_off = (lin[w] if w < len(lin) else lin[-1]) if lin else 0
    chunks = sorted(c for b in reg2bins(beg, max(end, beg + 1)) for c in ref["bins"].get(b, ()) if c[1] > min_off)
    out, done = [], 0  # done: rows below this virtual offset have been read
    for cb, ce in chunks:
        lo = bisect.bisect_left(data.vbeg, max(cb, done))
        hi = bisect.bisect_left(data.vbeg, ce)
        if hi > lo:
            m = (data.cid[lo:hi] == t) & (data.beg0[lo:hi] < end) & (data.end0[lo:hi] > beg)
            out += (np.nonzero(m)[0] + lo).tolist()
            done = max(done, ce)
    return out


def brute(data, name, beg, end):
    if name not in data.names:
        return []
    t = data.names.index(name)
    return np.nonzero((data.cid == t) & (data.beg0 < end) & (data.end0 > beg))[0].tolist()


def check_structure(tbi, data):
    """What any .tbi of a sorted file must satisfy."""
    assert (tbi["format"], tbi["col_seq"], tbi["col_beg"], tbi["col_end"], tbi["meta"], tbi["skip"]) == (2, 1, 2, 0, 35, 0)
    assert tbi["n_no_coor"] == 0
    assert tbi["names"] == data.names, (tbi["names"][:5], data.names[:5])  # the order of first appearance
    for t, ref in enumerate(tbi["refs"]):
        for b, chunks in ref["bins"].items():
            assert chunks, b
            for k, (cb, ce) in enumerate(chunks):
                assert cb < ce, (t, b, k)
                assert k == 0 or chunks[k - 1][1] <= cb, (t, b, k)  # ascending and disjoint
        lin = ref["lin"]
        assert all(lin[k] <= lin[k + 1] for k in range(len(lin) - 1)), t
        n_rows = int((data.cid == t).sum())
        assert ref["pseudo"] is not None and ref["pseudo"][2] == n_rows and ref["pseudo"][3] == 0, (t, ref["pseudo"], n_rows)
        mine = np.nonzero(data.cid == t)[0]
        assert ref["pseudo"][0] == data.vbeg[mine[0]] and ref["pseudo"][1] == data.vend[mine[-1]]
        assert len(lin) == int((data.end0[mine].max() - 1) >> 14) + 1
    for j in range(len(data.rows)):  # every row inside a chunk of exactly its bin
        chunks = tbi["refs"][int(data.cid[j])]["bins"].get(reg2bin(int(data.beg0[j]), int(data.end0[j])), ())
        k = bisect.bisect_right(chunks, (data.vbeg[j], 1 << 64)) - 1
        assert k >= 0 and chunks[k][0] <= data.vbeg[j] and data.vend[j] <= chunks[k][1], (j, data.rows[j][:60])
    # the linear index names, for every window, an offset at or below the first row that overlaps it
    for j in range(len(data.rows)):
        lin = tbi["refs"][int(data.cid[j])]["lin"]
        for w in {int(data.beg0[j]) >> 14, (int(data.end0[j]) - 1) >> 14}:
            assert lin[w] <= data.vbeg[j], (j, w)
