"""BGZF written on the GPU (k_bgzf_deflate and the piece pipeline,
bgzfwrite.hip): the kernel's bytes must be the host twin's bytes -- on the
payload grid in one launch and block by block, on whole files in one piece and
in many, through the project's own BGZF reader, and through the command line's
GROM_VCF_BGZF=1.  Python's zlib and gzip decode everything; the twin itself is
checked against them in test_bgzf_write_host.py."""
import gzip
import os
import random

import pytest

import _bgzf_write as W
from _util import CASES, GOLDEN_VCF, run_grom, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def grid():
    import grom_amd
    laid = W.payloads()
    return laid, grom_amd.bgzf_blocks([b for _, b in laid], device=None)


def test_grid_device_equals_twin(grid):
    import grom_amd
    laid, twin = grid
    dev = grom_amd.bgzf_blocks([b for _, b in laid], device=0)
    assert len(dev) == len(twin)
    diff = [name for (name, _), a, b in zip(laid, dev, twin) if a != b]
    assert not diff, diff[:10]
    for (name, b), blk in zip(laid, dev):
        W.check_block(name, b, blk)


@pytest.mark.parametrize("name", ["random0", "random1", "random65280", "zeros65280"])
def test_single_block_launch(grid, name):
    import grom_amd
    laid, twin = grid
    k = [n for n, _ in laid].index(name)
    dev = grom_amd.bgzf_blocks([laid[k][1]], device=0)
    assert dev == [twin[k]]
    W.check_block(name, laid[k][1], dev[0])


def _both(tmp_path, name, data):
    import grom_amd
    src = str(tmp_path / (name + ".in"))
    with open(src, "wb") as f:
        f.write(data)
    host, dev = str(tmp_path / (name + ".host.gz")), str(tmp_path / (name + ".dev.gz"))
    hs, ds = grom_amd.bgzf_compress(src, host), grom_amd.bgzf_compress(src, dev, device=0)
    assert open(dev, "rb").read() == open(host, "rb").read(), name
    assert open(dev + ".gzi", "rb").read() == open(host + ".gzi", "rb").read(), name
    same = ("blocks", "stored", "fixed", "dynamic", "literal_dynamic", "in_bytes", "out_bytes", "pieces")
    assert {k: ds[k] for k in same} == {k: hs[k] for k in same}, (ds, hs)
    assert gzip.decompress(open(dev, "rb").read()) == data
    return ds


@pytest.mark.parametrize("piece_kb", [None, 64])
def test_files_device_equals_twin(tmp_path, monkeypatch, piece_kb):
    W.tmp_env(monkeypatch, piece_kb)
    vcf = open(GOLDEN_VCF, "rb").read()
    mixed = vcf[:500000] + random.Random(3).randbytes(100000) + vcf[500000:900000]  # about 1 MB, a random stretch inside
    st = _both(tmp_path, "mixed", mixed)
    assert st["device_us"] > 0 and st["stored"] >= 1 and st["dynamic"] >= 10, st
    assert st["pieces"] > 10 if piece_kb else st["pieces"] == 1, st
    st = _both(tmp_path, "empty", b"")
    assert st["blocks"] == 0 and st["out_bytes"] == 28, st
    st = _both(tmp_path, "two", bytes(range(256)) * 255 + b"x")
    assert st["blocks"] == 2 and st["device_us"] > 0, st


def test_writer_on_the_device_does_not_depend_on_the_cuts(tmp_path, monkeypatch):
    import grom_amd
    W.tmp_env(monkeypatch, 128)
    data = open(GOLDEN_VCF, "rb").read()[:400000]
    want = str(tmp_path / "want.gz")
    with grom_amd.BgzfWriter(want) as w:
        w.write(data)
    for step in (7777, 100000):
        p = str(tmp_path / f"d{step}.gz")
        with grom_amd.BgzfWriter(p, device=0) as w:
            for i in range(0, len(data), step):
                w.write(data[i:i + step])
        assert w.stats["pieces"] == 4 and w.stats["device_us"] > 0, w.stats
        assert open(p, "rb").read() == open(want, "rb").read()
        assert open(p + ".gzi", "rb").read() == open(want + ".gzi", "rb").read()


def test_round_trip_through_the_fasta_reader(datadir, tmp_path):
    """A FASTA compressed on the device is read back by the device FASTA
    reader: the same table, the same bytes for entry 0."""
    import grom_amd
    _, fa = synth(datadir, "three_chr", CASES["three_chr"])
    gz = str(tmp_path / "r.fa.gz")
    st = grom_amd.bgzf_compress(fa, gz, device=0)
    assert st["in_bytes"] == os.path.getsize(fa)
    with grom_amd.FastaDevice(fa) as plain, grom_amd.FastaDevice(gz) as comp:
        assert comp.index() == plain.index()
        assert comp.load(0) == plain.load(0)


@pytest.mark.parametrize("case", ["three_chr", "sv"])
def test_cli_writes_bgzf(datadir, tmp_path, capfd, case):
    import grom_amd
    bam, fa = synth(datadir, case, CASES[case])
    plain, comp = tmp_path / "plain", tmp_path / "comp"
    plain.mkdir()
    comp.mkdir()
    run_grom(plain, bam, fa, "out.vcf")
    capfd.readouterr()
    run_grom(comp, bam, fa, "out.vcf", env_extra={"GROM_VCF_BGZF": "1"})
    out = capfd.readouterr().out
    rows, ctx = (plain / "out.vcf").read_bytes(), (plain / "out.ctx.vcf").read_bytes()
    assert sorted(os.listdir(comp)) == ["out.ctx.vcf.gz", "out.vcf.gz", "out.vcf.gz.gzi"]  # no plain file, nothing temporary
    assert gzip.decompress((comp / "out.vcf.gz").read_bytes()) == rows
    assert gzip.decompress((comp / "out.ctx.vcf.gz").read_bytes()) == ctx
    twin = str(tmp_path / "twin.gz")
    grom_amd.bgzf_compress(str(plain / "out.vcf"), twin, device=None)
    assert (comp / "out.vcf.gz").read_bytes() == open(twin, "rb").read()
    assert (comp / "out.vcf.gz.gzi").read_bytes() == open(twin + ".gzi", "rb").read()
    line = [l for l in out.splitlines() if l.startswith("BGZF output (device 0): ")]
    assert len(line) == 1 and "out.vcf.gz with out.vcf.gz.gzi" in line[0] and "out.ctx.vcf.gz" in line[0], out[-2000:]
    chk = grom_amd.bgzf_check(str(comp / "out.vcf.gz"), device=0)
    assert chk["ok"] and chk["eof_marker"] and chk["inflated_bytes"] == len(rows), chk
