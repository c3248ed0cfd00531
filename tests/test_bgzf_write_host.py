"""BGZF written by the compressor's host twin (CPU only).

The device compressor's algorithm (grom_amd/csrc/bgzfdef.h: the 64-position
match steps, the atomic-max hash table, the greedy parse, the length-limited
Huffman codes, the four priced candidates) runs on the host with the lanes as
loops (bgzfdef_host.cpp; device=None / -1 everywhere).  The yardstick is
Python's zlib and gzip: every block must inflate there to its payload, carry
zlib's CRC-32 and stay within payload + 31 bytes.  tools/deflate_check.cpp
repeats the grid under AddressSanitizer + UBSan with every buffer ending where
its data ends.  The GPU tests (test_bgzf_write_device.py) then demand the
twin's bytes from the kernel."""
import gzip
import os
import shutil
import subprocess

import pytest

import _bgzf_write as W
from _util import CASES, FILEDATE, GOLDEN_VCF, REPO, SEED, TILAPIA_FA, synth

# output bytes / Z1 measured for the twin; + 0.02 so that tuning the parse need not touch the test
VCF_RATIO = 0.9010
FASTA_RATIO = 0.9746
FASTA_ZFIXED = 1158437  # zlib level 6, Z_FIXED, per 65280-byte payload + 26


@pytest.fixture(scope="module")
def grid():
    import grom_amd
    laid = W.payloads()
    return laid, grom_amd.bgzf_blocks([b for _, b in laid], device=None)


def test_twin_grid_blocks_decode_with_zlib(grid):
    laid, blocks = grid
    assert len(blocks) == len(laid)
    btype = {name: W.check_block(name, b, blk) for (name, b), blk in zip(laid, blocks)}
    assert btype["random65280"] == 0  # stored
    assert len(blocks[[n for n, _ in laid].index("random65280")]) == 65280 + 31
    for name, t in btype.items():
        if name.startswith(("vcf", "fasta")):
            assert t == 2, (name, t)  # dynamic Huffman
    assert btype["fibonacci"] == 2
    # an empty payload is the EOF marker
    assert blocks[[n for n, _ in laid].index("random0")] == W.EOF_MARKER


def test_twin_grid_is_deterministic_and_alignment_free(grid):
    """The same payloads one by one, each at another start: the same bytes."""
    import grom_amd
    laid, blocks = grid
    for k, ((name, b), blk) in enumerate(zip(laid, blocks)):
        if len(b) > 5000 and not name.startswith(("random65280", "copies")):
            continue
        assert grom_amd.bgzf_blocks([b], device=None, lead=k % 16) == [blk], name


def test_blocks_refuses_a_long_payload():
    import grom_amd
    with pytest.raises(RuntimeError, match="65280"):
        grom_amd.bgzf_blocks([bytes(65281)], device=None)


def _compress(tmp_path, name, data, **kw):
    import grom_amd
    src, dst = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".gz"))
    with open(src, "wb") as f:
        f.write(data)
    st = grom_amd.bgzf_compress(src, dst, **kw)
    return dst, st


@pytest.mark.parametrize("what", ["empty", "two_blocks", "vcf", "fasta"])
def test_whole_files(tmp_path, monkeypatch, what):
    import grom_amd
    W.tmp_env(monkeypatch, None)
    data = {"empty": b"", "two_blocks": bytes(range(256)) * 255 + b"x", "vcf": open(GOLDEN_VCF, "rb").read(),
            "fasta": open(TILAPIA_FA, "rb").read()}[what]
    assert what != "two_blocks" or len(data) == 65281
    dst, st = _compress(tmp_path, what, data)
    out = open(dst, "rb").read()
    assert gzip.decompress(out) == data
    assert out[-28:] == W.EOF_MARKER
    blocks = W.walk(out)
    n_data = (len(data) + W.MAX - 1) // W.MAX
    assert len(blocks) == n_data + 1
    assert st["blocks"] == n_data == st["stored"] + st["fixed"] + st["dynamic"] + st["literal_dynamic"]
    assert st["in_bytes"] == len(data) and st["out_bytes"] == len(out) and st["device_us"] == 0
    chk = grom_amd.bgzf_check(dst)
    assert chk["ok"] and chk["eof_marker"] and chk["blocks"] == n_data + 1 and chk["inflated_bytes"] == len(data)
    # the .gzi: every block after the first (the EOF marker is not indexed)
    assert W.read_gzi(dst + ".gzi") == [(c, u) for c, u, _ in blocks[1:n_data]]
    assert not [f for f in os.listdir(tmp_path) if ".tmp." in f]
    # one payload per piece: the same bytes, the same index
    W.tmp_env(monkeypatch, 64)
    dst2, st2 = _compress(tmp_path, what + "_pieces", data)
    assert open(dst2, "rb").read() == out and open(dst2 + ".gzi", "rb").read() == open(dst + ".gzi", "rb").read()
    assert st2["pieces"] == n_data


def test_writer_does_not_depend_on_the_cuts(tmp_path, monkeypatch):
    import grom_amd
    W.tmp_env(monkeypatch, None)
    data = open(GOLDEN_VCF, "rb").read()[:150000]
    dst, _ = _compress(tmp_path, "whole", data)
    want, want_gzi = open(dst, "rb").read(), open(dst + ".gzi", "rb").read()
    for piece in (None, 64):
        W.tmp_env(monkeypatch, piece)
        for step in (1, 7, 100000):
            p = str(tmp_path / f"w{step}.gz")
            with grom_amd.BgzfWriter(p) as w:
                for i in range(0, len(data), step):
                    w.write(data[i:i + step])
            assert w.stats["in_bytes"] == len(data)
            assert open(p, "rb").read() == want and open(p + ".gzi", "rb").read() == want_gzi, (piece, step)
    # without an index: no .gzi
    p = str(tmp_path / "nogzi.gz")
    st = grom_amd.bgzf_compress(str(tmp_path / "whole.in"), p, gzi=False)
    assert open(p, "rb").read() == want and not os.path.exists(p + ".gzi") and st["blocks"] == 3


def test_writer_failure_leaves_no_file(tmp_path):
    import grom_amd
    with pytest.raises(RuntimeError):
        grom_amd.BgzfWriter(str(tmp_path / "no_such_dir" / "x.gz"))
    with pytest.raises(RuntimeError):
        grom_amd.bgzf_compress(str(tmp_path / "missing"), str(tmp_path / "y.gz"))
    assert os.listdir(tmp_path) == []


def test_size_against_zlib_level_1(tmp_path, monkeypatch):
    """Z1: zlib level 1 per 65280-byte payload + 26.  The VCF within 1.5 x Z1
    (Huffman-only coding is 3.3 x: a dead matcher cannot pass), the FASTA
    within zlib's Z_FIXED level 6 size (not without dynamic codes), and both
    within 0.02 of the ratio measured for the twin."""
    W.tmp_env(monkeypatch, None)
    vcf, fa = open(GOLDEN_VCF, "rb").read(), open(TILAPIA_FA, "rb").read()
    z1_vcf, z1_fa = W.z1_size(vcf), W.z1_size(fa)
    n_vcf = os.path.getsize(_compress(tmp_path, "vcf", vcf)[0]) - 28
    n_fa = os.path.getsize(_compress(tmp_path, "fa", fa)[0]) - 28
    print(f"VCF {n_vcf} B, Z1 {z1_vcf} B, ratio {n_vcf / z1_vcf:.4f}; FASTA {n_fa} B, Z1 {z1_fa} B, ratio {n_fa / z1_fa:.4f}")
    assert n_vcf <= 1.5 * z1_vcf
    assert n_fa <= FASTA_ZFIXED
    assert n_vcf / z1_vcf <= VCF_RATIO + 0.02
    assert n_fa / z1_fa <= FASTA_RATIO + 0.02


def test_deflate_check_under_sanitizer():
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = os.path.join("build", "san-asan", "deflate_check")
    r = subprocess.run(["make", "-s", exe, "SAN=asan"], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ)
    env.setdefault("ASAN_OPTIONS", "abort_on_error=0:detect_leaks=1")
    r = subprocess.run([os.path.join(REPO, exe)], cwd=REPO, env=env, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out and "runtime error" not in out, out[-6000:]
    assert r.returncode == 0, out[-6000:]
    assert "deflate_check: ok" in out, out[-6000:]


@pytest.mark.parametrize("how", ["child", "segs"])
def test_cli_refuses_what_needs_plain_offsets(datadir, tmp_path, capfd, how):
    """GROM_VCF_BGZF with -c or with GROM_VCF_SEGS: a message, a non-zero
    status, nothing written, before the BAM is even opened."""
    import grom_amd
    bam, fa = synth(datadir, "three_chr", CASES["three_chr"])
    env = {"GROM_FILEDATE": FILEDATE, "GROM_SEED": SEED, "GROM_VCF_BGZF": "1"}
    extra = []
    if how == "child":
        extra = ["-c", "0"]
    else:
        env["GROM_VCF_SEGS"] = str(tmp_path / "segs.txt")
    rc = grom_amd.cli_main(["-i", bam, "-r", fa, "-o", "refused.vcf"] + extra, env=env, cwd=str(tmp_path))
    out = capfd.readouterr().out
    assert rc != 0
    assert "GROM_VCF_BGZF cannot be combined with" in out and ("-c" if how == "child" else "GROM_VCF_SEGS") in out
    assert os.listdir(tmp_path) == []
