"""A plain gzip reference FASTA (one DEFLATE stream per member), CPU side
(DESIGN.md 4.7.1): the host twin of the device's parallel read -- guessed block
starts, the verifying chain, symbolic decode, the window hand-over, resolve and
CRC with one lane -- against Python's gzip module on every variant, chunk size
and guess mode; the conditions that keep it from passing through the sequential
path; the unit cap; the host route (zlib) behind GROM_FASTA_GZIP=1; the .info
round trip; and tools/gzip_check (good and damaged streams) under
AddressSanitizer + UBSan.  Without the switch a plain gzip file is refused
(tests/test_fasta_device.py)."""
import gzip
import os
import shutil
import subprocess

import pytest

from _gzip_variants import ALL_VARIANTS, EDGE_VARIANTS, files, plain_of, streams
from _util import CASES, GROM_BIN, REPO, synth
from test_fasta_device import _info_text, host_all


def _cases():
    for v in EDGE_VARIANTS:
        for chunk in (0, 4096, 1024, 256, 97):  # 0: the whole file is one chunk
            yield v, chunk
    yield "tilapia", 32768
    yield "tilapia", 8192


@pytest.mark.parametrize("variant,chunk", list(_cases()))
def test_twin_equals_gzip_decompress(variant, chunk):
    import grom_amd
    s, text = streams()[variant]
    assert gzip.decompress(s) == text
    for mode in (1, 0, 2):
        got, st = grom_amd.gzip_inflate_host(s, chunk, 0, mode)
        assert got == text, (variant, chunk, mode, st)
        assert st["members"] == (3 if variant == "three" else 1)
        if mode == 0:
            assert st["units"] == st["members"] and st["units_guessed"] == 0


def test_small_chunks_go_through_the_parallel_path():
    """memLevel 1 at 256-byte chunks: units shorter than the window, nearly every byte a window reference."""
    import grom_amd
    s, text = streams()["mem1"]
    got, st = grom_amd.gzip_inflate_host(s, 256, 0, 1)
    assert got == text
    print(st)
    assert st["units"] >= 90
    assert st["units_again"] * 50 <= st["units"]
    assert st["marker_bytes"] >= 60000
    assert st["groups"] > 1  # the hand-over's two levels are both used
    # deliberately wrong guesses: refused by the chain, the same bytes
    got2, st2 = grom_amd.gzip_inflate_host(s, 256, 0, 2)
    print(st2)
    assert got2 == text and st2["units_again"] >= 1 and st2["units_guessed"] == 0


def test_unit_cap_answers_host_only():
    import grom_amd
    s, _ = streams()["fixed"]
    with pytest.raises(grom_amd.FastaHostOnly):
        grom_amd.gzip_inflate_host(s, 1024, 4096, 1)


@pytest.mark.parametrize("variant", list(ALL_VARIANTS))
def test_gzip_through_the_host_path(datadir, monkeypatch, variant):
    monkeypatch.setenv("GROM_FASTA_GZIP", "1")
    paths = files(datadir)
    assert host_all(paths[variant]) == host_all(paths[plain_of(variant)])


def test_allow_gzip_switch(datadir, monkeypatch):
    import grom_amd
    monkeypatch.delenv("GROM_FASTA_GZIP", raising=False)
    paths = files(datadir)
    with pytest.raises(RuntimeError):
        grom_amd.fasta_index(paths["l1"])
    assert "recompress it with bgzip, or set GROM_FASTA_GZIP=1 to read it as it is" in grom_amd.last_error()
    assert "parallel" not in grom_amd.last_error()
    assert grom_amd.allow_gzip_fasta(True) is None
    try:
        assert grom_amd.fasta_index(paths["l1"]) == grom_amd.fasta_index(paths["plain"])
        monkeypatch.setenv("GROM_FASTA_GZIP", "1")
        assert grom_amd.allow_gzip_fasta(False) is True
        with pytest.raises(RuntimeError):  # refused whatever the environment says
            grom_amd.fasta_index(paths["l1"])
    finally:
        grom_amd.allow_gzip_fasta(None)
    assert grom_amd.fasta_index(paths["l1"])["n"] == 13  # the environment again


def test_info_of_a_gzip_file_loads_back(datadir, tmp_path):
    """<fasta>.info written for the .fa.gz by a plan-only run holds the plain
    file's table: file_pos are offsets in the inflated text."""
    bam0, fa0 = synth(datadir, "three_chr", CASES["three_chr"])
    with open(str(tmp_path / "r.fa.gz"), "wb") as f:
        f.write(gzip.compress(open(fa0, "rb").read(), 6))
    for n in ("", ".bai"):
        shutil.copy(bam0 + n, str(tmp_path / ("r.bam" + n)))
    env = dict(os.environ, GROM_PLAN_ONLY="1", GROM_FASTA_GZIP="1")
    out = []
    for k in range(2):  # the first run writes the file, the second reads it
        r = subprocess.run([GROM_BIN, "-i", "r.bam", "-r", "r.fa.gz", "-o", "o.vcf"], cwd=str(tmp_path), env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out.append(r.stdout)
        if k == 0:
            info = open(str(tmp_path / "r.fa.gz.info")).read()
            mt = os.path.getmtime(str(tmp_path / "r.fa.gz.info"))
    assert out[0] == out[1] and os.path.getmtime(str(tmp_path / "r.fa.gz.info")) == mt
    assert info == _info_text(fa0)


def test_gzip_check_under_sanitizer():
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = os.path.join("build", "san-asan", "gzip_check")
    r = subprocess.run(["make", "-s", exe, "SAN=asan"], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ)
    env.setdefault("ASAN_OPTIONS", "abort_on_error=0:detect_leaks=1")
    r = subprocess.run([os.path.join(REPO, exe)], cwd=REPO, env=env, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out and "runtime error" not in out, out[-6000:]
    assert r.returncode == 0, out[-6000:]
    assert "gzip_check ok" in out, out[-6000:]
