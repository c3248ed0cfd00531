"""Position-sorted, bgzipped, tabix-indexed VCF output: the host twin.

The sorting, indexing writer's algorithm (grom_amd/csrc/vcfsort.h: the rows'
facts, the key (contig id << 32) | POS, the virtual offsets from the BGZF
writer's fixed 65280-byte payloads, the bins; the runs through the BAI
accumulator) runs on the host as loops (vcfsort_host.cpp; device=None / -1
everywhere).  The yardsticks are Python's own sorted(), gzip, and the
independent tabix reader of _tabix.py: every output must inflate to the header
followed by the stably sorted rows, and every region query through the .tbi
must equal the brute-force answer.  tools/tbi_check.cpp repeats the grid under
AddressSanitizer + UBSan.  The GPU tests (test_vcf_tabix_device.py) then
demand the twin's bytes from the kernels."""
import gzip
import os
import shutil
import subprocess

import pytest

import _tabix as T
import _vcf_grid as G
from _util import CASES, FILEDATE, GOLDEN_CTX, GOLDEN_VCF, REPO, SEED, synth

GRID = G.grid()


def _run(tmp_path, name, text, device=None):
    import grom_amd
    src, dst = str(tmp_path / (name + ".vcf")), str(tmp_path / (name + ".vcf.gz"))
    with open(src, "wb") as f:
        f.write(text)
    return dst, grom_amd.vcf_tabix(src, dst, device=device)


def test_golden_vcf(tmp_path):
    text = open(GOLDEN_VCF, "rb").read()
    dst, st = _run(tmp_path, "golden", text)
    assert st["inversions"] >= 1, st  # (a sorted golden file would show nothing)
    assert st["rows"] == 20827 and st["contigs"] == 1 and st["radix_passes"] >= 1, st
    tbi, data = G.check_output(text, dst, st)
    # each <DEL> / <INV> span, asked on its own
    sym = [s for l, s in zip(data.rows, data.spans) if b"<DEL>" in l or b"<INV>" in l]
    assert sym
    for nm, _, b, e in sym:
        assert T.query(tbi, data, nm, b, e) == T.brute(data, nm, b, e)
    assert sorted(os.listdir(tmp_path)) == ["golden.vcf", "golden.vcf.gz", "golden.vcf.gz.gzi", "golden.vcf.gz.tbi"]


def test_golden_ctx_header_only(tmp_path):
    text = open(GOLDEN_CTX, "rb").read()
    assert all(l.startswith(b"#") for l in text.splitlines())
    dst, st = _run(tmp_path, "ctx", text)
    assert st["rows"] == 0 and st["contigs"] == 0, st
    assert T.parse_tbi(dst + ".tbi")["n_ref"] == 0
    assert gzip.decompress(open(dst, "rb").read()) == text
    G.check_output(text, dst, st)


@pytest.mark.parametrize("name", [n for n, _ in GRID])
def test_grid(tmp_path, name):
    text = dict(GRID)[name]
    dst, st = _run(tmp_path, name, text)
    G.check_output(text, dst, st)
    if name == "sorted":
        import grom_amd
        plain = str(tmp_path / "plain.gz")
        grom_amd.bgzf_compress(str(tmp_path / "sorted.vcf"), plain, device=None)
        assert open(dst, "rb").read() == open(plain, "rb").read()
        assert open(dst + ".gzi", "rb").read() == open(plain + ".gzi", "rb").read()
        assert st["inversions"] == 0, st
    if name == "one_pos":
        assert st["radix_passes"] == 0 and st["inversions"] == 0, st
    if name == "reverse":
        assert st["inversions"] >= 2000, st
    if name == "contigs300":
        assert st["contigs"] == 300 and st["radix_passes"] >= 3, st  # the contig id crosses a digit
    if name == "low_bits":
        assert st["radix_passes"] == 1, st
    if name == "high_bits":
        assert st["radix_passes"] == 1, st
    if name == "last_pos":
        assert st["linear_windows"] == 32768, st


@pytest.mark.parametrize("name", [n for n, _, _ in G.REFUSED])
def test_refusals(tmp_path, name):
    import grom_amd
    _, text, msg = [r for r in G.REFUSED if r[0] == name][0]
    d = tmp_path / "out"
    d.mkdir()
    src = str(tmp_path / "in.vcf")
    with open(src, "wb") as f:
        f.write(text)
    with pytest.raises(RuntimeError) as e:
        grom_amd.vcf_tabix(src, str(d / "o.vcf.gz"), device=None)
    assert msg in str(e.value), str(e.value)
    assert G.leftovers(d) == []


def test_independent_of_the_cuts(tmp_path, monkeypatch):
    import grom_amd
    text = dict(GRID)["rows4097"] + dict(GRID)["long_row"][len(G.HDR):]
    want = None
    for cut in (1, 7, 65281, len(text)):
        if cut == 7:
            monkeypatch.setenv("GROM_VCF_CHUNK_KB", "1")  # (the stream then also crosses many collecting chunks)
        else:
            monkeypatch.delenv("GROM_VCF_CHUNK_KB", raising=False)
        p = str(tmp_path / f"c{cut}.vcf.gz")
        with grom_amd.VcfWriter(p, device=None) as w:
            for i in range(0, len(text), cut):
                w.write(text[i:i + cut])
        assert w.stats["rows"] == 4097 + 4, w.stats
        if want is None:
            want = G.files(p)
            G.check_output(text, p, w.stats)
        assert G.files(p) == want, cut


def test_tbi_check_under_sanitizer(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = os.path.join("build", "san-asan", "tbi_check")
    r = subprocess.run(["make", "-s", exe, "SAN=asan"], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    grid_dir = tmp_path / "grid"
    grid_dir.mkdir()
    for name, text in GRID:
        (grid_dir / (name + ".vcf")).write_bytes(text)
    for name, text, _ in G.REFUSED:
        (grid_dir / ("refused_" + name + ".vcf")).write_bytes(text)
    env = dict(os.environ)
    env.setdefault("ASAN_OPTIONS", "abort_on_error=0:detect_leaks=1")
    r = subprocess.run([os.path.join(REPO, exe), str(grid_dir), GOLDEN_VCF], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=240)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out and "runtime error" not in out, out[-6000:]
    assert r.returncode == 0, out[-6000:]
    assert "tbi_check: ok" in out, out[-6000:]
    # the sanitized build wrote what the library writes
    import grom_amd
    for name in ("rows257", "levels", "long_row"):
        dst, _ = _run(tmp_path, "lib_" + name, dict(GRID)[name])
        assert G.files(dst) == G.files(str(grid_dir / (name + ".vcf.gz"))), name


@pytest.mark.parametrize("how", ["child", "segs", "tab_rows"])
def test_cli_refuses_before_any_file_or_device(datadir, tmp_path, capfd, how):
    """GROM_VCF_TABIX with -c, with GROM_VCF_SEGS or with -f: a message, a
    non-zero status, nothing written, before the BAM is even opened."""
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
