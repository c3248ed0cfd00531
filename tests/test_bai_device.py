"""The device index builder (grom_bai_build_device, baidev.hip): its file is
the host builder's (grom_bai_build, pinned by test_bai.py), byte for byte.

The generator starts a new block rather than split a record, starts every
chromosome on a new block and writes no unplaced records, so a helper
(tests/_handmade.py, zlib and struct only) inflates a generated BAM, may add
records built in Python, and deflates the stream again into BGZF blocks whose
payload sizes cycle through 997, 1, 4093, 65280, 37 bytes, with an empty block
after the 5th and the 200th block and the EOF block last: records and their
36-byte headers straddle blocks, record ends land on block ends and empty
blocks sit mid-file."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import pytest

from _handmade import EMPTY_AFTER, _header_len, _inflate, _rec, _records, _reblock
from _util import CASES, GROM_BIN, run_grom, synth

_cache = {}

UNPLACED = [_rec(-1, -1, b"u%d" % i, 4 | 8, (), 20, 0) for i in range(3)]


def _stream(datadir, case):
    if case not in _cache:
        bam, _ = synth(datadir, case, CASES[case])
        _cache[case] = _inflate(bam)
    return _cache[case]


def _reblocked_three_chr(datadir):
    """three_chr re-blocked with three unplaced records appended, and the host
    builder's index of it: made once, read by every test that needs it."""
    if "rb3" not in _cache:
        import grom_amd
        bam = os.path.join(str(datadir), "three_chr_reblocked.bam")
        nblk = _reblock(_stream(datadir, "three_chr") + b"".join(UNPLACED), bam)
        assert grom_amd.lib().grom_bai_build(bam.encode()) == 0
        _cache["rb3"] = (bam, nblk, open(bam + ".bai", "rb").read())
    return _cache["rb3"]


def _summary(path):
    import grom_amd
    out = (C.c_int64 * 5)()
    assert grom_amd.lib().grom_bai_summary(path.encode(), out) == 0
    return list(out)


def _both(bam, tmp_path):
    """The host builder's bytes for `bam` and the device builder's (written to a
    second path), with the device build's counters."""
    import grom_amd
    assert grom_amd.lib().grom_bai_build(bam.encode()) == 0
    want = open(bam + ".bai", "rb").read()
    dev = str(tmp_path / "device.bai")
    counters = grom_amd.bai_build(bam, dev)
    got = open(dev, "rb").read()
    assert [f for f in os.listdir(str(tmp_path)) if ".tmp." in f] == []
    return want, got, counters


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["three_chr", "empty_middle", "lowmapq_clip"])
def test_generated_files_byte_identical(datadir, tmp_path, case):
    bam0, _ = synth(datadir, case, CASES[case])
    bam = str(tmp_path / "x.bam")
    shutil.copy(bam0, bam)
    want, got, counters = _both(bam, tmp_path)
    assert got == want
    assert counters["records"] > 0 and counters["pieces"] >= 1 and counters["runs"] > 0


@pytest.mark.gpu
def test_reblocked_with_unplaced_byte_identical(datadir, tmp_path):
    import grom_amd
    bam0, nblk, want = _reblocked_three_chr(datadir)
    bam = str(tmp_path / "x.bam")
    shutil.copy(bam0, bam)
    counters = grom_amd.bai_build(bam)
    assert open(bam + ".bai", "rb").read() == want
    assert counters["blocks"] == nblk + len(EMPTY_AFTER) + 1
    assert _summary(bam + ".bai")[4] == 3
    seen = C.c_int64(0)
    bad = grom_amd.lib().grom_bai_selftest(bam.encode(), 200, 7, C.byref(seen))
    assert bad == 0 and seen.value > 0


@pytest.mark.gpu
@pytest.mark.parametrize("piece_kb,hook", [(64, False), (64, True), (2048, True)])
def test_small_pieces_and_wrong_guesses(datadir, tmp_path, monkeypatch, piece_kb, hook):
    """Records span pieces and runs continue across them (64 KB pieces: one
    walk group each; 2 MB pieces: the chain across groups too); with the hook
    every guess is a chunk's first byte."""
    import grom_amd
    bam, _, want = _reblocked_three_chr(datadir)
    monkeypatch.setenv("GROM_INDEX_PIECE_KB", str(piece_kb))
    if hook:
        monkeypatch.setenv("GROM_INDEX_GUESS", "2")
    dev = str(tmp_path / "device.bai")
    counters = grom_amd.bai_build(bam, dev)
    assert open(dev, "rb").read() == want
    assert counters["pieces"] > 10
    if hook:
        assert counters["chunks_rewalked"] > 0


@pytest.mark.gpu
def test_hand_made_records_byte_identical(datadir, tmp_path):
    s = _stream(datadir, "one_chr")
    h, _ = _header_len(s)
    last_pos = _records(s, h)[-1][3]
    first = [_rec(0, -1, b"neg", 0, ((30, "M"),), 30)]  # pos = -1 on a placed target
    tail = [_rec(0, last_pos, b"skip", 0, ((50, "M"), (40000, "N"), (50, "M")), 100),  # >= 3 windows, an upper-level bin
            _rec(0, last_pos + 5, b"nocigar", 0, (), 30)]  # no CIGAR, not flagged unmapped: end = pos + 1
    bam = str(tmp_path / "x.bam")
    _reblock(s[:h] + b"".join(first) + s[h:] + b"".join(tail), bam)
    want, got, counters = _both(bam, tmp_path)
    assert got == want
    assert counters["records"] == len(_records(s, h)) + 3


@pytest.mark.gpu
def test_header_only_bam(datadir, tmp_path):
    s = _stream(datadir, "three_chr")
    h, n_ref = _header_len(s)
    bam = str(tmp_path / "x.bam")
    _reblock(s[:h], bam)
    want, got, counters = _both(bam, tmp_path)
    assert got == want == b"BAI\x01" + struct.pack("<i", n_ref) + bytes(8 * n_ref) + bytes(8)
    assert counters["records"] == 0


@pytest.mark.gpu
def test_unsorted_file_fails_and_leaves_nothing(datadir, tmp_path):
    import grom_amd
    s = _stream(datadir, "one_chr")
    h, _ = _header_len(s)
    recs = _records(s, h)
    i = next(k for k in range(len(recs) // 2, len(recs) - 1) if recs[k][2] == recs[k + 1][2] and recs[k][3] < recs[k + 1][3])
    (a, la, _, _), (b, lb, _, _) = recs[i], recs[i + 1]
    bam = str(tmp_path / "x.bam")
    _reblock(s[:a] + s[b:b + lb] + s[a:a + la] + s[b + lb:], bam)
    assert grom_amd.lib().grom_bai_build(bam.encode()) != 0
    if os.path.exists(bam + ".bai"):
        os.remove(bam + ".bai")
    dev = str(tmp_path / "device.bai")
    with pytest.raises(RuntimeError, match="sorted"):
        grom_amd.bai_build(bam, dev)
    assert os.listdir(str(tmp_path)) == ["x.bam"]


@pytest.mark.gpu
def test_cli_builds_a_missing_index(datadir, tmp_path, capfd):
    import grom_amd
    bam0, fa0 = synth(datadir, "one_chr", CASES["one_chr"])
    for d in ("with", "without"):
        os.mkdir(str(tmp_path / d))
        shutil.copy(bam0, str(tmp_path / d / "y.bam"))
        shutil.copy(fa0, str(tmp_path / d / "y.fa"))
    shutil.copy(bam0 + ".bai", str(tmp_path / "with" / "y.bam.bai"))
    flush = C.CDLL(None).fflush  # the CLI runs in this process: its stdio buffer
    run_grom(tmp_path / "with", "y.bam", "y.fa", "y.vcf")
    flush(None)
    capfd.readouterr()
    run_grom(tmp_path / "without", "y.bam", "y.fa", "y.vcf", env_extra={"GROM_BUILD_INDEX": "1"})
    flush(None)
    out = capfd.readouterr().out
    assert sum(1 for l in out.splitlines() if l.startswith("built y.bam.bai on device")) == 1
    for name in ("y.vcf", "y.ctx.vcf"):
        assert open(str(tmp_path / "without" / name)).read() == open(str(tmp_path / "with" / name)).read()
    assert open(str(tmp_path / "without" / "y.bam.bai"), "rb").read() == open(bam0 + ".bai", "rb").read()
    # a second run finds the file and builds nothing
    run_grom(tmp_path / "without", "y.bam", "y.fa", "y2.vcf", env_extra={"GROM_BUILD_INDEX": "1"})
    flush(None)
    assert "built y.bam.bai" not in capfd.readouterr().out


def test_cli_without_the_variable_still_refuses(datadir, tmp_path):
    bam0, fa0 = synth(datadir, "one_chr", CASES["one_chr"])
    shutil.copy(bam0, str(tmp_path / "y.bam"))
    shutil.copy(fa0, str(tmp_path / "y.fa"))
    r = subprocess.run([GROM_BIN, "-i", "y.bam", "-r", "y.fa", "-o", "y.vcf"], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "Could not open BAM indexing file" in r.stdout
    assert not os.path.exists(str(tmp_path / "y.bam.bai"))
    # a file that is there but does not load is never replaced
    open(str(tmp_path / "y.bam.bai"), "wb").write(b"BAI\x01\xff")
    r = subprocess.run([GROM_BIN, "-i", "y.bam", "-r", "y.fa", "-o", "y.vcf"], cwd=str(tmp_path),
                       env=dict(os.environ, GROM_BUILD_INDEX="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Could not open BAM indexing file" in r.stdout
    assert open(str(tmp_path / "y.bam.bai"), "rb").read() == b"BAI\x01\xff"


def test_helper_file_and_no_device(datadir, tmp_path):
    """The helper's file is one the host builder indexes, with the figures of
    the original (51 bins, 81 chunks, 39 linear intervals) and the three
    unplaced records; without a device the device builder says so and leaves
    no file (with one, its file is the host's)."""
    import grom_amd
    bam0, _ = synth(datadir, "three_chr", CASES["three_chr"])
    bam, nblk, want = _reblocked_three_chr(datadir)
    assert nblk == 2364
    assert _summary(bam0 + ".bai")[:4] == [3, 51, 81, 39]
    assert _summary(bam + ".bai") == [3, 51, 81, 39, 3]
    dev = str(tmp_path / "device.bai")
    out = (C.c_int64 * 8)()
    rc = grom_amd.lib().grom_bai_build_device(bam.encode(), dev.encode(), 0, out)
    if rc == 0:
        assert open(dev, "rb").read() == want
    else:
        assert rc < 0 and grom_amd.last_error() != ""
        assert os.listdir(str(tmp_path)) == []
