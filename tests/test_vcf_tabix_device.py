"""Position-sorted, bgzipped, tabix-indexed VCF output on the GPU (the kernels
of vcfsort.hip): the device's three files must be the host twin's, byte for
byte -- on the hand-made grid, on the golden VCF, whatever the BGZF writer's
piece size and the collecting chunks -- the independent tabix reader's queries
must hold on the device's files, and the command line's GROM_VCF_TABIX=1 must
write them.  The twin itself is checked against Python's sort, gzip and
_tabix.py in test_vcf_tabix_host.py."""
import gzip
import os

import pytest

import _bgzf_write as W
import _tabix as T
import _vcf_grid as G
from _util import CASES, FILEDATE, GOLDEN_CTX, GOLDEN_VCF, SEED, run_grom, run_oracle, synth

pytestmark = pytest.mark.gpu

GRID = G.grid()


def _both(tmp_path, name, text):
    import grom_amd
    src = str(tmp_path / (name + ".vcf"))
    with open(src, "wb") as f:
        f.write(text)
    host, dev = str(tmp_path / (name + ".host.vcf.gz")), str(tmp_path / (name + ".dev.vcf.gz"))
    hs, ds = grom_amd.vcf_tabix(src, host, device=None), grom_amd.vcf_tabix(src, dev, device=0)
    for a, b, what in zip(G.files(dev), G.files(host), ("data", ".tbi", ".gzi")):
        assert a == b, (name, what)
    same = ("rows", "header_lines", "contigs", "inversions", "radix_passes", "bins", "chunks", "linear_windows")
    assert {k: ds[k] for k in same} == {k: hs[k] for k in same}, (ds, hs)
    assert ds["lines_us"] > 0 and ds["sort_us"] > 0 and ds["index_us"] > 0, ds
    return dev, ds


@pytest.mark.parametrize("name", [n for n, _ in GRID])
def test_grid_device_equals_twin(tmp_path, name):
    text = dict(GRID)[name]
    dev, st = _both(tmp_path, name, text)
    G.check_output(text, dev, st)
    assert sorted(os.listdir(tmp_path)) == sorted(
        [name + ".vcf"] + [f"{name}.{w}.vcf.gz{s}" for w in ("host", "dev") for s in ("", ".tbi", ".gzi")])


def test_golden_device_equals_twin_and_answers_queries(tmp_path):
    text = open(GOLDEN_VCF, "rb").read()
    dev, st = _both(tmp_path, "golden", text)
    assert st["inversions"] >= 1 and st["rows"] == 20827, st
    tbi, data = G.check_output(text, dev, st)
    for l, (nm, _, b, e) in zip(data.rows, data.spans):
        if b"<DEL>" in l or b"<INV>" in l:
            assert T.query(tbi, data, nm, b, e) == T.brute(data, nm, b, e)
    ctx = open(GOLDEN_CTX, "rb").read()
    dev, st = _both(tmp_path, "ctx", ctx)
    assert st["rows"] == 0 and T.parse_tbi(dev + ".tbi")["n_ref"] == 0
    assert gzip.decompress(open(dev, "rb").read()) == ctx


@pytest.mark.parametrize("name", [n for n, _, _ in G.REFUSED])
def test_device_refuses_what_the_twin_refuses(tmp_path, name):
    import grom_amd
    _, text, msg = [r for r in G.REFUSED if r[0] == name][0]
    d = tmp_path / "out"
    d.mkdir()
    src = str(tmp_path / "in.vcf")
    with open(src, "wb") as f:
        f.write(text)
    with pytest.raises(RuntimeError) as e:
        grom_amd.vcf_tabix(src, str(d / "o.vcf.gz"), device=0)
    assert msg in str(e.value), str(e.value)
    assert G.leftovers(d) == []


def test_piece_size_and_chunks_do_not_matter(tmp_path, monkeypatch):
    import grom_amd
    text = open(GOLDEN_VCF, "rb").read()[:1_500_000]
    text = text[:text.rindex(b"\n") + 1] + dict(GRID)["long_row"][len(G.HDR):]
    want = None
    for piece_kb, chunk_kb, cut in ((None, None, len(text)), (63.75, None, 100_000), (None, 64, 7777), (63.75, 1, 65281)):
        W.tmp_env(monkeypatch, piece_kb)
        if chunk_kb is None:
            monkeypatch.delenv("GROM_VCF_CHUNK_KB", raising=False)
        else:
            monkeypatch.setenv("GROM_VCF_CHUNK_KB", str(chunk_kb))
        p = str(tmp_path / f"p{piece_kb}_{chunk_kb}.vcf.gz")
        with grom_amd.VcfWriter(p, device=0) as w:
            for i in range(0, len(text), cut):
                w.write(text[i:i + cut])
        if want is None:
            want = G.files(p)
            G.check_output(text, p, w.stats, full_queries=False)
        assert G.files(p) == want, (piece_kb, chunk_kb)
    monkeypatch.delenv("GROM_VCF_CHUNK_KB", raising=False)
    W.tmp_env(monkeypatch, None)
    host = str(tmp_path / "host.vcf.gz")
    with grom_amd.VcfWriter(host, device=None) as w:
        w.write(text)
    assert G.files(host) == want


@pytest.mark.parametrize("case", ["three_chr", "sv"])
def test_cli_writes_sorted_indexed_vcf(datadir, tmp_path, capfd, case):
    bam, fa = synth(datadir, case, CASES[case])
    plain, tab, ora = tmp_path / "plain", tmp_path / "tab", tmp_path / "ora"
    for d in (plain, tab, ora):
        d.mkdir()
    run_grom(plain, bam, fa, "out.vcf")
    run_oracle(ora, bam, fa, "out.vcf")
    # without the variable: the plain outputs, as before
    assert sorted(os.listdir(plain)) == ["out.ctx.vcf", "out.vcf"]
    for f in ("out.vcf", "out.ctx.vcf"):
        assert (plain / f).read_bytes() == (ora / f).read_bytes(), f
    capfd.readouterr()
    run_grom(tab, bam, fa, "out.vcf", env_extra={"GROM_VCF_TABIX": "1"})
    out = capfd.readouterr().out
    assert sorted(os.listdir(tab)) == sorted(f"{b}.gz{s}" for b in ("out.vcf", "out.ctx.vcf") for s in ("", ".tbi", ".gzi"))
    for f in ("out.vcf", "out.ctx.vcf"):
        text = (plain / f).read_bytes()
        tbi, data = G.check_output(text, str(tab / (f + ".gz")), full_queries=False)
        hdr, rows, _ = T.sorted_text(text)
        got = gzip.decompress((tab / (f + ".gz")).read_bytes())
        assert got.startswith(hdr) and sorted(got[len(hdr):].splitlines(True)) == sorted(rows)
    assert len(T.sorted_text((plain / "out.vcf").read_bytes())[1]) > 100
    line = [l for l in out.splitlines() if l.startswith("Sorted, indexed output (device 0): ")]
    assert len(line) == 1 and "out.vcf.gz with out.vcf.gz.tbi and out.vcf.gz.gzi" in line[0] and "out.ctx.vcf.gz" in line[0], out[-2000:]


@pytest.mark.parametrize("how", ["child", "segs", "tab_rows"])
def test_cli_refusals(datadir, tmp_path, capfd, how):
    import grom_amd
    bam, fa = synth(datadir, "three_chr", CASES["three_chr"])
    env = {"GROM_FILEDATE": FILEDATE, "GROM_SEED": SEED, "GROM_VCF_TABIX": "1"}
    extra, word = [], None
    if how == "child":
        extra, word = ["-c", "0"], "-c"
    elif how == "segs":
        env["GROM_VCF_SEGS"] = str(tmp_path / "segs.txt")
        word = "GROM_VCF_SEGS"
    else:
        extra, word = ["-f"], "-f"
    rc = grom_amd.cli_main(["-i", bam, "-r", fa, "-o", "refused.vcf"] + extra, env=env, cwd=str(tmp_path))
    out = capfd.readouterr().out
    assert rc != 0
    assert "GROM_VCF_TABIX cannot be combined with " + word in out, out[-1000:]
    assert os.listdir(tmp_path) == []
