"""A plain gzip reference FASTA read on the device (gzipdev.hip, DESIGN.md
4.7.1) behind GROM_FASTA_GZIP=1: the index and every load equal the host's on
every variant and at small chunks; the statistics show that the parallel path
was taken (and that wrong guesses are refused and decoded again); the unit cap
answers "host only" and the CLI then reads on the host; a wrong CRC-32 or ISIZE
fails the open by name; a whole CLI run gives the plain file's rows."""
import ctypes as C
import shutil
import struct
import subprocess

import pytest

from _gzip_variants import ALL_VARIANTS, files, plain_of, streams
from _util import CASES, GROM_BIN, run_grom, synth
from test_fasta_device import _device_equals_host, _read, _strip, host_all

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _gzip_on(monkeypatch):
    monkeypatch.setenv("GROM_FASTA_GZIP", "1")


def _equals_host(path, ref_path):
    """_device_equals_host; for a file with fewer entries than its adopted-table
    part loads (the one-entry tilapia contig), the same checks on the entries it has."""
    import grom_amd
    table, loads = host_all(ref_path)
    if table["n"] >= 8:
        return _device_equals_host(path, ref_path)
    with grom_amd.FastaDevice(path, 0) as f:
        got = f.index()
        assert _strip(got) == table
        assert [e["load_len"] for e in got["entries"]] == [len(b) for b in loads]
        for i, want in enumerate(loads):
            assert f.load(i) == want, table["entries"][i]["name"]
    with grom_amd.FastaDevice(path, 0) as f:
        f.set_index(table)
        for i in reversed(range(table["n"])):
            assert f.load_len(i) == len(loads[i])
            assert f.load(i) == loads[i]


@pytest.mark.parametrize("variant,chunk_kb", [(v, None) for v in ALL_VARIANTS] +
                         [("mem1", "0.25"), ("mem1", "1"), ("three", "0.25"), ("three", "1"), ("tilapia", "8")])
def test_gzip_device_equals_host(datadir, monkeypatch, variant, chunk_kb):
    import grom_amd
    if chunk_kb:
        monkeypatch.setenv("GROM_GZIP_CHUNK_KB", chunk_kb)
    paths = files(datadir)
    _equals_host(paths[variant], paths[plain_of(variant)])
    with grom_amd.FastaDevice(paths[variant], 0) as f:
        assert f.kind == "gzip" and not f.bgzf
        st = f.gzip_stats()
        assert st["members"] == (3 if variant == "three" else 1)
    with grom_amd.FastaDevice(paths[plain_of(variant)], 0) as f:
        assert f.kind == "plain"


@pytest.mark.parametrize("mode", ["1", "0", "2"])
def test_guess_modes(datadir, monkeypatch, mode):
    import grom_amd
    monkeypatch.setenv("GROM_GZIP_CHUNK_KB", "0.25")
    monkeypatch.setenv("GROM_GZIP_GUESS", mode)
    paths = files(datadir)
    _device_equals_host(paths["mem1"], paths["plain"])
    with grom_amd.FastaDevice(paths["mem1"], 0) as f:
        st = f.gzip_stats()
    print(st)
    host = grom_amd.gzip_inflate_host(streams()["mem1"][0], 256, 0, int(mode))[1]
    for k in ("units", "units_guessed", "units_again", "marker_bytes", "members", "max_unit_bytes", "groups"):
        assert st[k] == host[k], k  # the twin runs the same stages
    if mode == "1":
        assert st["units"] >= 90
        assert st["units_again"] * 50 <= st["units"]
        assert st["marker_bytes"] >= 60000
    elif mode == "0":
        assert st["units"] == 1 and st["units_guessed"] == 0
    else:
        assert st["units_again"] >= 1 and st["units_guessed"] == 0


def test_unit_cap_is_host_only(datadir, tmp_path, monkeypatch):
    import grom_amd
    monkeypatch.setenv("GROM_GZIP_UNIT_MAX_KB", "4")
    paths = files(datadir)
    with pytest.raises(grom_amd.FastaHostOnly):
        grom_amd.FastaDevice(paths["fixed"], 0)
    # the CLI takes the host route and gives the plain file's rows
    bam0, fa0 = synth(datadir, "one_chr", CASES["one_chr"])
    for n in ("", ".bai"):
        shutil.copy(bam0 + n, str(tmp_path / ("y.bam" + n)))
    shutil.copy(fa0, str(tmp_path / "y.fa"))
    import zlib
    c = zlib.compressobj(6, zlib.DEFLATED, 31, 8, zlib.Z_FIXED)
    with open(str(tmp_path / "y.fa.gz"), "wb") as f:
        f.write(c.compress(open(fa0, "rb").read()) + c.flush())
    import os
    env = dict(os.environ, GROM_FILEDATE="20260101", GROM_SEED="7")
    r = subprocess.run([GROM_BIN, "-i", "y.bam", "-r", "y.fa.gz", "-o", "g.vcf"], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "reading y.fa.gz on the host" in r.stderr
    r = subprocess.run([GROM_BIN, "-i", "y.bam", "-r", "y.fa", "-o", "p.vcf"], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for ext in (".vcf", ".ctx.vcf"):
        assert _read(tmp_path / ("g" + ext), True) == _read(tmp_path / ("p" + ext), True)
    assert any(not l.startswith("#") for l in _read(tmp_path / "p.vcf"))


@pytest.mark.parametrize("field,word", [("crc", "CRC-32"), ("isize", "ISIZE")])
def test_trailer_checks(tmp_path, field, word):
    """Valid DEFLATE whose last member's trailer is wrong: the open fails and names the member and the check."""
    import grom_amd
    s = bytearray(streams()["three"][0])
    crc, isize = struct.unpack("<II", s[-8:])
    s[-8:] = struct.pack("<II", crc ^ 0x5a5a, isize) if field == "crc" else struct.pack("<II", crc, isize + 1)
    p = str(tmp_path / "bad.fa.gz")
    with open(p, "wb") as f:
        f.write(s)
    with pytest.raises(RuntimeError) as e:
        grom_amd.FastaDevice(p, 0)
    assert not isinstance(e.value, grom_amd.FastaHostOnly)
    assert word in grom_amd.last_error() and "member 3" in grom_amd.last_error()


def test_cli_three_chr_with_a_plain_gzip_reference(datadir, tmp_path, capfd):
    import gzip
    bam0, fa0 = synth(datadir, "three_chr", CASES["three_chr"])
    for n in ("", ".bai"):
        shutil.copy(bam0 + n, str(tmp_path / ("three_chr.bam" + n)))
    shutil.copy(fa0, str(tmp_path / "three_chr.fa"))
    with open(str(tmp_path / "three_chr.fa.gz"), "wb") as f:
        f.write(gzip.compress(open(fa0, "rb").read(), 6))
    run_grom(tmp_path, "three_chr.bam", "three_chr.fa", "p.vcf")
    flush = C.CDLL(None).fflush  # the CLI runs in this process: its stdio buffers
    capfd.readouterr()
    run_grom(tmp_path, "three_chr.bam", "three_chr.fa.gz", "g.vcf", env_extra={"GROM_VERBOSE": "1"})
    flush(None)
    err = capfd.readouterr().err
    assert "device FASTA loader (gzip" in err and "gzip on the device" in err
    for ext in (".vcf", ".ctx.vcf"):
        assert _read(tmp_path / ("g" + ext), True) == _read(tmp_path / ("p" + ext), True)
    assert "##reference=three_chr.fa.gz\n" in _read(tmp_path / "g.vcf")
    assert any(not l.startswith("#") for l in _read(tmp_path / "g.vcf"))
