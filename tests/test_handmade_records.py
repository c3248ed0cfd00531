"""Parity on records and block layouts the generator never writes.

Every other parity test feeds the scan a BAM written by grom_synth: S/M/I/D
CIGARs, paired reads, two quality values, short names, no aux but SA:Z, one
record per block boundary.  Here the inputs are the hand-made records of
tests/_handmade.py (CIGAR ops N H P = X and more than 1,000 of them, all 16
base codes, quality and MAPQ edges, long / empty / prefix names, unpaired
reads, secondary / supplementary / QC-fail / duplicate flags, every aux value
type, reads over the contig's ends) merged into a small generated BAM, and the
re-blocked three_chr and sv files (records and their headers straddling BGZF
blocks, chromosomes changing mid-block, 1-byte and empty blocks, an unplaced
tail).

The CPU tests come first: the oracle under AddressSanitizer + UBSan on the
hand-made file (its expected values do not come from reads outside its
arrays), the witness rule (every group of records changes the oracle's dump
inside its own window -- a record that changes nothing tests nothing), and
the two host decoders against each other and against the oracle's walk.  The
GPU tests compare the product with the oracle, bit-exact, through every
decoder mode and forced scan route.

Group 10 of the list this file was written from (l_seq = 0 with a CIGAR; a
CIGAR that consumes more query than l_seq) is left out, and group 3's reads
are at most 1,000 bases long: for those records GROM.c reads outside its own
arrays (GROM.c:6800, 6806 past l_seq; cdp_seq's 1,000 entries, GROM.c:1514,
6761-6766) and has no defined answer (handmade_records' docstring).
Group 13's records before the scan's first base are skipped by the reference
whatever precedes them (GROM.c:6406: every record before g_one_base_rd_len / 4
+ 1); their witness is the skip count, which moves the ring index of every
later base, and the group has records on both sides of that base."""
import os
import re
import subprocess

import numpy as np
import pytest

import _handmade as H
from _util import CASES, GROM_BIN, REPO, load_counts, load_indels, run, run_grom, run_oracle
from test_host import parse_meta, parse_plan

ORACLE_SAN = os.path.join(REPO, "oracle", "grom_oracle_san")
# group 5 names -b 25, group 6 -q 10, group 9 -M, group 11 -S
WITNESS_SETS = {"default": [], "S": ["-S"], "M": ["-M"], "q10b25": ["-q", "10", "-b", "25"]}
GPU_SETS = dict(WITNESS_SETS, n2=["-n", "2"], f=["-f"])
DECODE_MODES = {"0": {"GROM_DEVICE_DECODE": "0"}, "1": {"GROM_DEVICE_DECODE": "1"},
                "3w": {"GROM_DEVICE_DECODE": "1", "GROM_DD_WORKERS": "3"},
                "g0": {"GROM_DEVICE_DECODE": "1", "GROM_WS_GUESS": "0"},
                "g2": {"GROM_DEVICE_DECODE": "1", "GROM_WS_GUESS": "2"},
                "cu": {"GROM_DEVICE_DECODE": "1", "GROM_COPY_TILES": "1", "GROM_TEST_CP_UNSTAGED": "1"},
                "pc": {"GROM_DEVICE_DECODE": "1", "GROM_DD_PIECE_MB": "0.0625"},
                "pcu": {"GROM_DEVICE_DECODE": "1", "GROM_DD_PIECE_MB": "0.0625", "GROM_COPY_TILES": "1"}}
_done = {}


def _oracle(datadir, key, bam, fa, extra):
    """One oracle run with a dump per (input, flags) and session: the dump
    prefix, the VCF name and the run's stdout."""
    tag = f"hmo_{key}{''.join(extra).replace('-', '_')}"
    if tag not in _done:
        r = run_oracle(datadir, bam, fa, f"{tag}.vcf", extra, dump=str(datadir / tag))
        _done[tag] = r.stdout
    return tag, _done[tag]


def _reblocked(datadir, case):
    """A generated case re-blocked (three_chr with the unplaced tail of
    test_bai_device.py), indexed by the host builder."""
    key = "rb_" + case
    if key not in _done:
        stream = H.inflated(datadir, case, CASES[case])
        if case == "three_chr":
            stream += b"".join(H._rec(-1, -1, b"u%d" % i, 4 | 8, (), 20, 0) for i in range(3))
        bam, nblk = H.reblocked(datadir, case + "_rb", stream)
        assert nblk > 100
        _done[key] = (bam, os.path.join(str(datadir), case + ".fa"))
    return _done[key]


def _input(datadir, which):
    if which == "handmade":
        c = H.handmade_case(datadir)
        return c["bam"], c["fa"]
    return _reblocked(datadir, which)


# ------------------------------------------------------------------ CPU tests
def test_fixture_records_are_well_formed(datadir):
    """The hand-made file read back: every record's fields fit its block_size,
    records are sorted within their contig, the count is what was built, and
    the reference under every group's aligned bases is A/C/G/T where the
    group's mismatches are meant to be real ones."""
    import struct
    c = H.handmade_case(datadir)
    s = H._inflate(c["bam"])
    h, n_ref = H._header_len(s)
    recs = H._records(s, h)
    base = H.inflated(datadir, "hm_base", H.BASE_ARGS)
    n_base = len(H._records(base, H._header_len(base)[0]))
    assert len(recs) == n_base + c["n"] and 40 < c["n"] < 100
    keys = [(tid, pos) for _, _, tid, pos in recs]
    assert keys == sorted(keys)
    for o, n, tid, pos in recs:
        lqn, _, _, nc, flag, lq = struct.unpack_from("<BBHHHi", s, o + 12)
        assert lqn >= 1 and s[o + 36 + lqn - 1] == 0
        assert 36 + lqn + 4 * nc + (lq + 1) // 2 + lq <= n
        if not flag & 0x4:
            assert nc > 0 and lq <= 1000  # no mapped record without a CIGAR, none above cdp_seq's size
    ref = H.read_fasta(c["fa"])[0][1].upper()
    for g, wins in c["groups"].items():
        if g not in (12, 13):
            for lo, hi in wins:
                assert set(ref[lo + H.REACH:hi - H.REACH]) <= set("ACGT"), g
    flat = sorted((w, g) for g, ws in c["groups"].items() for w in ws)
    for ((_, hi), g0), ((lo, _), g1) in zip(flat, flat[1:]):
        assert g0 == g1 or hi <= lo, (g0, g1)  # windows of different groups never overlap


@pytest.mark.parametrize("opts", ["default", "S"])
def test_sanitizer_oracle_runs_clean(datadir, opts):
    """The oracle CLI built with AddressSanitizer and UBSan (oracle/Makefile
    grom_oracle_san, a stand-alone program) on the hand-made BAM: exit 0, no
    report, and the plain build's rows."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(REPO, "oracle"), "grom_oracle_san"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    bam, fa = _input(datadir, "handmade")
    extra = WITNESS_SETS[opts]
    r = run(ORACLE_SAN, ["-i", bam, "-r", fa, "-o", f"san_{opts}.vcf"] + extra, str(datadir),
            {"ASAN_OPTIONS": "abort_on_error=0:detect_leaks=1"})
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out and "runtime error" not in out, out[-6000:]
    tag, _ = _oracle(datadir, "handmade", bam, fa, extra)
    for ext in (".vcf", ".ctx.vcf"):
        assert open(datadir / f"san_{opts}{ext}").read() == open(datadir / f"{tag}{ext}").read()


def _dump(datadir, tag, chrom, chr_len):
    import grom_amd
    cnt = load_counts(datadir / f"{tag}.{chrom}.cnt")
    ind = load_indels(datadir / f"{tag}.{chrom}.ind")
    sv = np.fromfile(datadir / f"{tag}.{chrom}.sv", dtype=grom_amd.SV_DTYPE)
    caf = np.fromfile(datadir / f"{tag}.{chrom}.caf", np.int32).reshape(3, chr_len)
    return cnt, ind, sv, caf


def _stats(stdout):
    m = re.search(r"insert mean, insert minimum, insert maximum: (\d+) (\d+) (\d+)", stdout)
    return [int(x) for x in m.groups()]


@pytest.mark.parametrize("opts", list(WITNESS_SETS))
def test_every_group_changes_the_oracle_dump(datadir, opts):
    """The witness rule.  Oracle dumps of the generated BAM and of the
    hand-made one: inside its own windows every group changes a .cnt row, an
    .ind or .sv record or a .caf base (under every option set here, the ones
    groups 5, 6, 9 and 11 name included); outside all windows no .cnt row and
    no .caf base differs, so a window's difference is its group's.  The
    hand-made records leave the insert mean and maximum alone (they set the
    window geometry and the scan's first base, _handmade.SCAN_START); the
    unpaired reads enter the sample with their lengths (GROM.c:1205-1318) and
    lower the minimum.  Three records lie before the scan's first base and are
    skipped; the records at the contig's end extend the evaluated range."""
    c = H.handmade_case(datadir)
    extra = WITNESS_SETS[opts]
    tb, out_b = _oracle(datadir, "base", c["base"], c["fa"], extra)
    th, out_h = _oracle(datadir, "handmade", c["bam"], c["fa"], extra)
    (mean_b, min_b, max_b), (mean_h, min_h, max_h) = _stats(out_b), _stats(out_h)
    assert (mean_b, max_b) == (mean_h, max_h) and min_h < min_b
    assert max(8 * (2 * mean_h - 1), 8 * (max_h + 1)) * 2 // 4 + 1 == H.SCAN_START  # GROM.c:22282-22290, 2918
    meta_b, meta_h = parse_meta(datadir / f"{tb}.{c['chrom']}.meta"), parse_meta(datadir / f"{th}.{c['chrom']}.meta")
    assert meta_b["n_skip"] == 0 and meta_h["n_skip"] == 3
    assert meta_h["p_end"] > c["chr_len"] - 1000 > meta_b["p_end"]
    cb, ib, sb, fb = _dump(datadir, tb, c["chrom"], c["chr_len"])
    ch, ih, sh, fh = _dump(datadir, th, c["chrom"], c["chr_len"])
    # rows of the bases both runs evaluated, by position
    lo, hi = max(cb[0, 0], ch[0, 0]), min(cb[-1, 0], ch[-1, 0])
    assert lo == H.SCAN_START and (cb[:, 0] == np.arange(cb[0, 0], cb[-1, 0] + 1)).all()
    rb, rh = cb[lo - cb[0, 0]:hi + 1 - cb[0, 0]], ch[lo - ch[0, 0]:hi + 1 - ch[0, 0]]
    cnt_diff = np.zeros(c["chr_len"], bool)
    cnt_diff[lo:hi + 1] = (rb != rh).any(axis=1)
    caf_diff = (fb != fh).any(axis=0)
    inside = np.zeros(c["chr_len"], bool)
    for g, wins in sorted(c["groups"].items()):
        changed = []
        for w0, w1 in wins:
            inside[w0:w1] = True
            changed.append(cnt_diff[w0:w1].any() or caf_diff[w0:w1].any())
            for a, b in ((ib, ih), (sb, sh)):
                wa = a[(a["pos"] >= w0) & (a["pos"] < w1) & (a["pos"] <= hi)]
                wb = b[(b["pos"] >= w0) & (b["pos"] < w1) & (b["pos"] <= hi)]
                changed.append(wa.tobytes() != wb.tobytes())
        assert any(changed), f"group {g} changes nothing under {extra}"
        if g not in (12, 13):  # (their reference is N: only depth can change)
            assert any(cnt_diff[w0:w1].any() for w0, w1 in wins), g
    assert not (cnt_diff & ~inside).any(), np.nonzero(cnt_diff & ~inside)[0][:5]
    assert not (caf_diff & ~inside).any(), np.nonzero(caf_diff & ~inside)[0][:5]
    if opts == "M":
        # of the five records at one start position, the flagged duplicate is
        # dropped always and -M drops rm_second alone: four reads more than the
        # generated BAM at their common base by default, three under -M
        td, _ = _oracle(datadir, "handmade", c["bam"], c["fa"], [])
        tbd, _ = _oracle(datadir, "base", c["base"], c["fa"], [])
        p, rc_all = H.RMDUP_POS + 7, 15
        row = lambda tag: load_counts(datadir / f"{tag}.{c['chrom']}.cnt")[p - H.SCAN_START]
        assert row(td)[0] == p
        assert row(td)[rc_all] - row(tbd)[rc_all] == 4 and row(th)[rc_all] - row(tb)[rc_all] == 3


def _plans(datadir, bam, fa, extra, tag):
    base = ["-i", bam, "-r", fa, "-o", f"pd_{tag}.vcf"] + extra
    ser = run(GROM_BIN, base, str(datadir), {"GROM_PLAN_ONLY": "1", "GROM_SERIAL_DECODE": "1"})
    want = sorted(l for l in ser.stdout.splitlines() if l.startswith("plan "))
    assert want
    for thr, recs in (("1", "1000"), ("4", "777"), ("3", "65536")):
        r = run(GROM_BIN, base, str(datadir), {"GROM_PLAN_ONLY": "1", "GROM_DECODE_THREADS": thr,
                                               "GROM_PIECE_RECS": recs, "GROM_VERBOSE": "1"})
        assert "streamed decode:" in r.stdout, r.stdout[-2000:]
        got = sorted(l for l in r.stdout.splitlines() if l.startswith("plan "))
        assert got == want, (thr, got, want)
    return parse_plan(ser.stdout)


def _plan_matches_oracle(datadir, plan, tag):
    assert plan
    for name, p in plan.items():
        meta = parse_meta(datadir / f"{tag}.{name}.meta")
        assert p["n_skip"] == meta["n_skip"], (name, p, meta)
        if p["p_last"] >= 0:
            assert p["p_last"] + 1 == meta["p_end"], (name, p, meta)
        else:
            assert meta["n_ingested"] == 0


@pytest.mark.parametrize("which,opts", [("handmade", "default"), ("handmade", "S"), ("handmade", "M"),
                                        ("three_chr", "default")],
                         ids=["handmade", "handmade_S", "handmade_M", "three_chr_reblocked"])
def test_host_decoders_agree_and_match_oracle_walk(datadir, which, opts):
    """As test_streamed_decode_matches_serial_reader and
    test_stream_plan_matches_oracle_walk (tests/test_host.py), on the hand-made
    and the re-blocked files: the threaded decoder's plan lines (stream facts
    and digests of every staged array) equal the serial reader's in all three
    thread / piece settings, and each chromosome's skip prefix and last base
    are the oracle's."""
    bam, fa = _input(datadir, which)
    extra = WITNESS_SETS[opts]
    plan = _plans(datadir, bam, fa, extra, f"{which}_{opts}")
    tag, _ = _oracle(datadir, which, bam, fa, extra)
    _plan_matches_oracle(datadir, plan, tag)
    if which == "handmade":
        assert plan["chr1"]["n_skip"] == 3


# ------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("opts", list(GPU_SETS))
def test_handmade_counters_and_vcf_bit_exact(datadir, opts):
    """.cnt, .caf, .ind, .sv, the VCF and .ctx.vcf of the hand-made BAM are
    the oracle's (test_gpu_parity's comparison)."""
    from test_gpu_parity import _check_counters_files
    bam, fa = _input(datadir, "handmade")
    _check_counters_files(datadir, bam, fa, None, GPU_SETS[opts], f"hm_{opts}")


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["GROM_MEM_SLOTS", "GROM_HEAVY_TILES"])
def test_handmade_forced_scan_routes(datadir, route):
    """The global-slot kernel and the heavy-tile route (k_scan_tile_mem),
    forced for every tile of the hand-made BAM."""
    from test_gpu_parity import _check_counters_files
    bam, fa = _input(datadir, "handmade")
    _check_counters_files(datadir, bam, fa, None, [], f"hm_{route.lower()}", env_extra={route: "1"})


def _outputs_are_the_oracles(datadir, tag, g):
    for ext in (".vcf", ".ctx.vcf"):
        assert open(datadir / f"{tag}{ext}").read() == open(datadir / f"{g}{ext}").read(), (g, ext)


@pytest.mark.gpu
def test_handmade_serial_reader_path(datadir):
    """The serial reader (GROM_SERIAL_DECODE=1) on the hand-made BAM."""
    bam, fa = _input(datadir, "handmade")
    tag, _ = _oracle(datadir, "handmade", bam, fa, [])
    run_grom(datadir, bam, fa, "g_hm_ser.vcf", [], env_extra={"GROM_SERIAL_DECODE": "1"})
    _outputs_are_the_oracles(datadir, tag, "g_hm_ser")


def _stage_lines(datadir, capfd, which, opts, mode):
    """One CLI run in a decoder mode: its sorted "stage" digest lines; the
    outputs are checked against the oracle's."""
    key = ("stage", which, opts, mode)
    if key not in _done:
        bam, fa = _input(datadir, which)
        extra = WITNESS_SETS[opts]
        tag, _ = _oracle(datadir, which, bam, fa, extra)
        capfd.readouterr()
        g = f"g{mode}_{which}_{opts}"
        run_grom(datadir, bam, fa, f"{g}.vcf", extra,
                 env_extra=dict(DECODE_MODES[mode], GROM_STAGE_DIGEST="1", GROM_VERBOSE="1"))
        out = capfd.readouterr().out
        assert ("device decode:" in out) == (mode != "0"), out[-1500:]
        if mode == "3w":
            assert " 3 decode workers," in out, out[-1500:]
        _outputs_are_the_oracles(datadir, tag, g)
        _done[key] = sorted(l for l in out.splitlines() if l.startswith("stage "))
    return _done[key]


@pytest.mark.gpu
@pytest.mark.parametrize("opts", ["default", "S"])
@pytest.mark.parametrize("mode", ["0", "1", "g0", "g2", "cu", "pc", "pcu"])
def test_handmade_through_the_decoders(datadir, capfd, mode, opts):
    """The scheme of test_device_decode_matches_host_decode on the hand-made
    BAM: in every decoder mode the staged input (GROM_STAGE_DIGEST lines:
    stream facts, every array, CIGAR / base / quality / SA-XP content, dropped
    records, the name-id relation) is the host decoder's, and the outputs are
    the oracle's."""
    host = _stage_lines(datadir, capfd, "handmade", opts, "0")
    assert host
    assert _stage_lines(datadir, capfd, "handmade", opts, mode) == host


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["0", "1", "3w", "g2", "pc"])
def test_reblocked_three_chr_through_the_decoders(datadir, capfd, mode):
    """The same on three_chr re-blocked: records and their 36-byte headers
    straddle blocks, chromosomes change mid-block, 1-byte and empty blocks sit
    mid-file and three unplaced records end it."""
    host = _stage_lines(datadir, capfd, "three_chr", "default", "0")
    assert host
    assert _stage_lines(datadir, capfd, "three_chr", "default", mode) == host


@pytest.mark.gpu
def test_reblocked_three_chr_counters_bit_exact(datadir):
    from test_gpu_parity import _check_counters_files
    bam, fa = _input(datadir, "three_chr")
    _check_counters_files(datadir, bam, fa, "three_chr", [], "rb_three_chr")


@pytest.mark.gpu
def test_reblocked_sv_with_S(datadir):
    """The re-blocked sv case (SA:Z records and their headers straddling
    blocks) with -S, through the default device decode."""
    bam, fa = _input(datadir, "sv")
    tag, _ = _oracle(datadir, "sv", bam, fa, ["-S"])
    run_grom(datadir, bam, fa, "g_rb_sv_S.vcf", ["-S"])
    _outputs_are_the_oracles(datadir, tag, "g_rb_sv_S")
    assert sum(1 for l in open(datadir / "g_rb_sv_S.vcf") if not l.startswith("#")) > 100
