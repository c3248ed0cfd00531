"""BAM/BGZF helpers (zlib and struct only) and the hand-made records.

grom_synth writes only S/M/I/D CIGARs, paired reads with two quality values
and short names, starts a new BGZF block rather than split a record and
starts every chromosome on a new block.  The helpers here inflate a generated
BAM, build records in Python, merge them into the generated ones and deflate
the stream again into BGZF blocks whose payload sizes cycle through 997, 1,
4093, 65280, 37 bytes, with an empty block after the 5th and the 200th block
and the EOF block last: records and their 36-byte headers straddle blocks,
record ends land on block ends, chromosomes change mid-block and empty blocks
sit mid-file.

handmade_case() is the input of tests/test_handmade_records.py: the records of
RECORD GROUPS below merged into `grom_synth -L 60000,30000 -s 61`."""
import os
import struct
import zlib

from _util import synth

PAYLOADS = (997, 1, 4093, 65280, 37)
EMPTY_AFTER = (5, 200)
NT16 = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"


def _inflate(path):
    d = open(path, "rb").read()
    out, o = [], 0
    while o < len(d):
        assert d[o:o + 4] == b"\x1f\x8b\x08\x04"
        xlen, = struct.unpack_from("<H", d, o + 10)
        bsize = None
        x = o + 12
        while x < o + 12 + xlen:
            si1, si2, slen = struct.unpack_from("<BBH", d, x)
            if (si1, si2, slen) == (66, 67, 2):
                bsize, = struct.unpack_from("<H", d, x + 4)
            x += 4 + slen
        out.append(zlib.decompress(d[o + 12 + xlen:o + bsize + 1 - 8], -15))
        o += bsize + 1
    return b"".join(out)


def _block(payload):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    z = c.compress(payload) + c.flush()
    assert len(z) + 26 <= 65536
    return (struct.pack("<4BI2BH2B2H", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(z) + 25) + z +
            struct.pack("<II", zlib.crc32(payload), len(payload)))


def _reblock(stream, path):
    """The stream as BGZF blocks of the cycling payload sizes; returns the
    number of blocks that hold data."""
    blocks, o, k = [], 0, 0
    while o < len(stream):
        n = PAYLOADS[k % len(PAYLOADS)]
        blocks.append(_block(stream[o:o + n]))
        o += n
        k += 1
        if k in EMPTY_AFTER:
            blocks.append(_block(b""))
    blocks.append(_block(b""))  # the EOF block
    open(path, "wb").write(b"".join(blocks))
    return k


def _header_len(s):
    assert s[:4] == b"BAM\x01"
    l_text, = struct.unpack_from("<i", s, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", s, o)
    o += 4
    for _ in range(n_ref):
        ln, = struct.unpack_from("<i", s, o)
        o += 4 + ln + 4
    return o, n_ref


def _records(s, o):
    """(offset, length with block_size, tid, pos) of every record from o on."""
    out = []
    while o < len(s):
        bs, tid, pos = struct.unpack_from("<iii", s, o)
        out.append((o, 4 + bs, tid, pos))
        o += 4 + bs
    assert o == len(s)
    return out


def _reg2bin(beg, end):
    """SAM v1 section 5.3."""
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def _rec(tid, pos, name, flag, cigar=(), l_seq=0, mapq=30, seq=None, qual=None, mtid=-1, mpos=-1, tlen=0, aux=b"",
         bin_=4680):
    """One BAM record.  `name` may hold a NUL (l_read_name then exceeds the
    name's C length); `seq` is text over the 16 base codes (without it the
    read has l_seq '=' codes); `qual` a sequence of l_seq values (without it
    every quality is 255, "absent"); `aux` the raw bytes of the aux area."""
    qn = name + b"\0"
    assert len(qn) <= 255
    cig = b"".join(struct.pack("<I", n << 4 | CIGAR_OPS.index(op)) for n, op in cigar)
    if seq is not None:
        l_seq = len(seq)
    sb = bytearray((l_seq + 1) // 2)
    for k, ch in enumerate(seq or ""):
        sb[k >> 1] |= NT16.index(ch) << (0 if k & 1 else 4)
    q = b"\xff" * l_seq if qual is None else bytes(qual)
    assert len(q) == l_seq
    body = (struct.pack("<iiBBHHHiiii", tid, pos, len(qn), mapq, bin_, len(cigar), flag, l_seq, mtid, mpos, tlen) + qn +
            cig + bytes(sb) + q + aux)
    return struct.pack("<i", len(body)) + body


def merge(stream, records):
    """`records` (BAM records as bytes) merged into the records of `stream`
    (an inflated BAM), each into its contig, in position order; stable: where
    positions tie, the stream's records come first and `records` keep their
    order.  Unplaced records (tid -1) go last.  Returns the new stream."""
    h, n_ref = _header_len(stream)
    every = [stream[o:o + n] for o, n, _, _ in _records(stream, h)] + list(records)

    def key(r):
        tid, pos = struct.unpack_from("<ii", r, 4)
        return (tid if tid >= 0 else n_ref, pos)
    return stream[:h] + b"".join(sorted(every, key=key))


def read_fasta(path):
    """[(name, sequence as written)] of a FASTA file."""
    out = []
    for line in open(path):
        if line.startswith(">"):
            out.append([line[1:].split()[0], []])
        else:
            out[-1][1].append(line.strip())
    return [(n, "".join(s)) for n, s in out]


# ---------------------------------------------------------------- RECORD GROUPS
BASE_ARGS = ["-L", "60000,30000", "-s", "61"]
# the generated chr1 is N in [0, 10000) and [50000, 60000), reads lie between
PAIRED_F = 0x1 | 0x40 | 0x20  # paired, first, mate reverse; never "proper": outside the insert-size sample
PAIRED_R = 0x1 | 0x40 | 0x10
# The scan starts at base g_one_base_rd_len / 4 + 1 (GROM.c:2918) and skips
# every record before it (GROM.c:6406); with this input's insert statistics
# (mean 498, maximum 666) that is 8 * (2 * 498 - 1) / 2 + 1.  The test checks it.
SCAN_START = 3981
RMDUP_POS = 32300  # group 9's -M start-position group
REACH = 800  # bases either side of a record that it can change: above the insert maximum, below the groups' spacing


def _other(c):
    return "ACGT"[("ACGT".index(c) + 1) % 4] if c in "ACGT" else "A"


def _query(ref, pos, cigar, mism=()):
    """Read bases for `cigar` at `pos`: the reference's under M/=/X (A past the
    contig end), ACGT... for inserted and TGCA... for clipped bases; the query
    offsets of `mism` then get another base."""
    q, x = [], pos
    for n, op in cigar:
        if op in "M=X":
            q.append(ref[x:x + n].upper().ljust(n, "A"))
            x += n
        elif op == "I":
            q.append(("ACGT" * (n // 4 + 1))[:n])
        elif op == "S":
            q.append(("TGCA" * (n // 4 + 1))[:n])
        elif op in "DN":
            x += n
    q = list("".join(q))
    for k in mism:
        q[k] = _other(q[k])
    return "".join(q)


def _cig(text):
    """'10S40=2I48X' -> ((10, 'S'), ...)."""
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append((int(n), ch))
            n = ""
    return tuple(out)


def _ref_len(cigar):
    return sum(n for n, op in cigar if op in "MDN=X")


def handmade_records(ref, chr_len):
    """The hand-made records for contig 0 (reference text `ref`): a list of
    (group, record) and {group: [(lo, hi)]}, the windows a group's records can
    change.  Groups are numbered as in the list below; each sits at least 1 kb
    from the next, so the first differing base of a failure names the group.

     1  = and X: single-op reads (the scan's fast path), both strands, and
        inside a multi-op CIGAR
     2  N, P, H: 5H30M500N2P30M7H; H then S, and the mirror; N before I and D
     3  more than 1,000 CIGAR ops (GROM.c:6740-6750 copies 1,000: the tail is
        missing from the tally, the clip lengths and the read end, but not from
        the depth arrays, GROM.c:6605-6671), with twins of 1,000 and 1,001
     4  all 16 base codes; a read of '=' codes
     5  qualities 0, 1, 19-21 (-b 20), 24-26 (-b 25), 93, 254, 255
     6  MAPQ 0, 1, 9-11 (-q 10), 19-21 (-q 20), 254, 255
     7  names: equal 49-, 50- and 254-character names, empty names, names that
        differ only at byte 40, lengths 31/32/33 of one prefix, a proper
        prefix, l_read_name past the first NUL
     8  unpaired reads, 25S51M25S (odd l_seq), both strands
     9  flags 0x100, 0x800, 0x200 (kept), 0x400, 0x4 (dropped); a -M
        start-position group with a paired 0x400 record and unpaired twins
    11  aux: every value type before SA:Z, "SA" inside a Z value, XP and SA,
        a d value, aux areas of 99 and 100 bytes, an SA with missing fields
    12  contig end: 50M ending at len-2, len-1, len, len+5; 10M5D40M 30 before
        the end; a mate on the second contig; mtid -1 without the unmapped flag
    13  contig start: soft-clipped reads at 0, 1 (clip position -1) and on
        both sides of the scan's first base

    No group 10 (l_seq = 0 with a CIGAR, a CIGAR that consumes more query
    than l_seq): GROM.c:6800 reads cdp_qual[cdp_snv_base] and GROM.c:6806
    cdp_seq[cdp_snv_base] for every base the CIGAR aligns, so past l_seq it
    reads the record's aux bytes or the buffer behind the record and the
    bases an earlier read left in cdp_seq: the reference has no defined
    answer for such a record.  For the same reason no read here is longer than
    cdp_seq's 1,000 entries (GROM.c:888, 1514, 6761-6766): group 3 gets its ops
    from 1M1D pairs, not from 700 insertions."""
    out, win = [], {}

    def add(group, pos, cigar, name, flag=PAIRED_F, mism=(), seq=None, qual=None, mapq=60, aux=b"", mate=None, q=40):
        cigar = _cig(cigar) if isinstance(cigar, str) else tuple(cigar)
        if seq is None:
            seq = _query(ref, pos, cigar, mism)
        if qual is None:
            qual = [q] * len(seq)
        if mate is None:
            if not flag & 0x1:
                mate = (-1, -1, 0)
            elif flag & 0x10:
                mate = (0, pos - 300, -450)
            else:
                mate = (0, pos + 300, 450)
        span = max(_ref_len(cigar), 1)
        out.append((group, _rec(0, pos, name, flag, cigar, 0, mapq, seq, qual, mate[0], mate[1], mate[2], aux,
                                _reg2bin(pos, pos + span))))
        # a read reaches from its left clip to its mate (the pair binning, GROM.c:8388-8525)
        win.setdefault(group, []).append((max(pos - REACH, 0), min(pos + span + REACH, chr_len)))

    # 1
    p = 11000
    add(1, p, "100=", b"eq_f", PAIRED_F, [10])
    add(1, p + 10, "100=", b"eq_r", PAIRED_R, [20])
    add(1, p + 20, "100X", b"x_f", PAIRED_F, [30])
    add(1, p + 30, "100X", b"x_r", PAIRED_R, [40])
    add(1, p + 200, "10S40=2I48X", b"eq_x_multi", PAIRED_F, [15, 60])
    # 2
    p = 13500
    add(2, p, "5H30M500N2P30M7H", b"nph", PAIRED_F, [5, 40])
    add(2, p + 700, "5H10S40M", b"h_then_s", PAIRED_R, [12])
    add(2, p + 710, "40M10S5H", b"s_then_h", PAIRED_F, [3])
    add(2, p + 750, "20M50N3I27M", b"n_then_i", PAIRED_F, [4, 30])
    add(2, p + 760, "20M50N4D30M", b"n_then_d", PAIRED_R, [4, 30])
    # 3
    p = 16000
    add(3, p, [(1, "M"), (1, "I")] * 100 + [(1, "M"), (1, "D")] * 600 + [(5, "M")], b"ops1401", PAIRED_F, [0, 400, 803])
    add(3, p + 1500, [(5, "S")] + [(1, "M"), (1, "I")] * 100 + [(1, "M"), (1, "D")] * 399 + [(1, "M")], b"ops1000",
        PAIRED_F, [5, 604])
    add(3, p + 3000, [(1, "M"), (1, "I")] * 100 + [(1, "M"), (1, "D")] * 400 + [(5, "M")], b"ops1001", PAIRED_R,
        [0, 603])
    # 4
    p = 22000
    add(4, p, "16M", b"codes16", PAIRED_F, seq=NT16)
    add(4, p + 4, "16M", b"codes16r", PAIRED_R, seq=NT16[::-1])
    add(4, p + 100, "50M", b"only_eq", PAIRED_F, seq="=" * 50)
    # 5
    p = 24000
    quals = [0, 1, 19, 20, 21, 24, 25, 26, 93, 254, 255]
    add(5, p, "11M", b"quals_match", PAIRED_F, qual=quals)
    add(5, p, "11M", b"quals_mism", PAIRED_F, range(11), qual=quals)
    add(5, p + 2, "11M", b"quals_mism_r", PAIRED_R, range(11), qual=quals[::-1])
    # 6
    p = 26000
    for k, mq in enumerate((0, 1, 9, 10, 11, 19, 20, 21, 254, 255)):
        add(6, p + 3 * k, "60M", b"mapq%d" % mq, PAIRED_R if k & 1 else PAIRED_F, [30 - 3 * k], mapq=mq)
    # 7: every set of names has its own mismatching base (base p + 2 + 4 * set)
    p = 28000
    names = [(b"n" * 49,) * 2, (b"m" * 50,) * 2, (b"z" * 254,) * 2, (b"",) * 2,
             (b"q" * 40 + b"a" + b"q" * 5, b"q" * 40 + b"b" + b"q" * 5), (b"r" * 31, b"r" * 32, b"r" * 33),
             (b"pre", b"prefix"), (b"nul\0xx", b"nul\0yy", b"nul")]
    for k, group_names in enumerate(names):
        for nm in group_names:
            add(7, p, "50M", nm, PAIRED_F, [2 + 4 * k])
    # 8
    p = 30000
    add(8, p, "25S51M25S", b"unpaired_f", 0, [30])
    add(8, p + 10, "25S51M25S", b"unpaired_r", 16, [31])
    # 9
    p = RMDUP_POS - 300
    for k, fl in enumerate((0x100, 0x800, 0x200, 0x400, 0x4)):
        add(9, p + 5 * k, "40M", b"flag%x" % fl, PAIRED_F | fl, [20 - 5 * k])
    add(9, p + 300, "60M", b"rm_first", PAIRED_F, [7])
    add(9, p + 300, "60M", b"rm_dupflag", PAIRED_F | 0x400, [7])
    add(9, p + 300, "60M", b"rm_second", PAIRED_F, [7])  # -M drops it (GROM.c:6432-6588)
    add(9, p + 300, "60M", b"rm_unpaired1", 0, [9])
    add(9, p + 300, "60M", b"rm_unpaired2", 0, [9])  # not paired: -M keeps it
    # 11: 60M40S, forward, the rest of the read 200 bases on (a split-read deletion, GROM.c:7431-7945)
    p = 34500
    every_type = (b"NMi" + struct.pack("<i", 3) + b"XAA!" + b"XBBc" + struct.pack("<i", 3) + b"\1\2\3" + b"XSBS" +
                  struct.pack("<iHH", 2, 1, 2) + b"XFf" + struct.pack("<f", 1.5) + b"MDZ50A49\0" + b"XHH1AE3\0")

    def sa(pos):
        return b"SAZchr1,%d,+,60S40M,60,0;\0" % (pos + 260 + 1)

    def pad_to(aux, n):
        return b"COZ" + b"x" * (n - len(aux) - 4) + b"\0" + aux
    auxes = [every_type + sa(p), b"COZxSAZy\0" + sa(p + 20),
             b"XPZchr1,+%d,60S40M,60,0;\0" % (p + 40 + 261) + sa(p + 40),
             b"XDd" + struct.pack("<d", 2.5) + sa(p + 60), pad_to(sa(p + 80), 99), pad_to(sa(p + 100), 100),
             b"SAZchr1,%d\0" % (p + 120 + 261)]
    assert len(auxes[0]) < 100 and len(auxes[4]) == 99 and len(auxes[5]) == 100
    for k, aux in enumerate(auxes):
        add(11, p + 20 * k, "60M40S", b"aux%d" % k, PAIRED_F, [3], aux=aux, mate=(0, p + 20 * k + 500, 650))
    # 12
    for k, end in enumerate((chr_len - 2, chr_len - 1, chr_len, chr_len + 5)):
        add(12, end - 49, "50M", b"end%d" % k, PAIRED_F, [1])
    add(12, chr_len - 30, "10M5D40M", b"end_two_blocks", PAIRED_F, [1])
    add(12, 43000, "20S80M", b"mate_chr2", PAIRED_R, [25], mate=(1, 12000, 0))
    add(12, 43010, "80M20S", b"mate_none", PAIRED_F, [5], mate=(-1, -1, 0))
    # 13
    add(13, 0, "10S40M", b"start0", PAIRED_F, [12])
    add(13, 1, "10S40M", b"start1", PAIRED_F, [12])
    add(13, SCAN_START - 1, "10S40M", b"before_scan", PAIRED_F, [12])
    add(13, SCAN_START, "10S40M", b"scan_first", PAIRED_F, [12])
    add(13, SCAN_START + 1, "10S40M", b"scan_second", PAIRED_R, [12])
    assert len(out) < 100
    return out, win


_cache = {}


def inflated(datadir, name, args):
    """The inflated stream of a generated BAM (made once)."""
    if name not in _cache:
        bam, _ = synth(datadir, name, args)
        _cache[name] = _inflate(bam)
    return _cache[name]


def reblocked(datadir, name, stream):
    """`stream` as <name>.bam in the cycling block sizes, with the host
    builder's index (grom_bai_build, pinned by test_bai.py): (path, data blocks)."""
    import grom_amd
    bam = os.path.join(str(datadir), name + ".bam")
    nblk = _reblock(stream, bam)
    assert grom_amd.lib().grom_bai_build(bam.encode()) == 0
    return bam, nblk


def handmade_case(datadir):
    """{"base": the generated BAM, "bam": the hand-made one (re-blocked,
    indexed), "fa", "groups": {group: windows}, "n": hand-made records,
    "chr_len"}, made once per session."""
    if "hm" not in _cache:
        base, fa = synth(datadir, "hm_base", BASE_ARGS)
        stream = inflated(datadir, "hm_base", BASE_ARGS)
        name, ref = read_fasta(fa)[0]
        recs, groups = handmade_records(ref, len(ref))
        bam, _ = reblocked(datadir, "hm_made", merge(stream, [r for _, r in recs]))
        _cache["hm"] = {"base": base, "bam": bam, "fa": fa, "groups": groups, "n": len(recs), "chr_len": len(ref),
                        "chrom": name.lower(), "records": recs}
    return _cache["hm"]
