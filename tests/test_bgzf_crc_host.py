"""BGZF block checksums on the host (CPU only).

The device kernel's algorithm (grom_amd/csrc/bgzfcrc.h: a block striped over
64 lanes in 16-byte chunks, slicing-by-16, the skip table, the GF(2)
multiplications, the combine) runs on the host with the lanes as a loop
(grom_bgzf_crc_twin) and must give zlib's CRC-32 exactly; tools/crc_check.cpp
does the same under AddressSanitizer + UBSan with every block at the end of
its heap buffer.  grom_bgzf_check is the host file check; GROM_VERIFY_CRC=1 /
grom_bgzf_verify(1) makes the host readers (the decoder threads, the serial
reader, the index builder) fail on a block whose bytes are not its CRC-32's --
damage that inflates to the right length and that nothing noticed before."""
import os
import random
import shutil
import subprocess
import zlib

import pytest

import _bgzf
from _util import CASES, GROM_BIN, REPO, synth


def test_crc_twin_matches_zlib():
    """The grid's lengths and 65535, 65536 (no BGZF payload once compressed:
    raw buffers only) x start alignments 0..15 x random, 0x00, 0xff bytes: the
    twin's CRC-32 equals zlib.crc32.  The block ends where the buffer ends
    (cap = off + n), so the twin's bounded loads are exercised too."""
    import grom_amd
    twin = grom_amd.lib().grom_bgzf_crc_twin
    rng = random.Random(5)
    bad = []
    for n in _bgzf.GRID + (65535, 65536):
        for fill in _bgzf.FILLS:
            for a in range(16):
                buf = bytes(0xa5 ^ i for i in range(a)) + _bgzf.fill_bytes(fill, n, rng)
                got = twin(buf, len(buf), a, n)
                if got != zlib.crc32(buf[a:]):
                    bad.append((n, fill, a, hex(got)))
    assert not bad, bad[:10]
    # a block inside a larger buffer: the bytes after it do not count
    buf = rng.randbytes(70000)
    for n in (1, 17, 1008, 4093, 60000):
        for a in range(16):
            assert twin(buf, len(buf), 3000 + a, n) == zlib.crc32(buf[3000 + a:3000 + a + n]), (n, a)


def test_crc_check_under_sanitizer():
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = os.path.join("build", "san-asan", "crc_check")
    r = subprocess.run(["make", "-s", exe, "SAN=asan"], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ)
    env.setdefault("ASAN_OPTIONS", "abort_on_error=0:detect_leaks=1")
    r = subprocess.run([os.path.join(REPO, exe)], cwd=REPO, env=env, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out and "runtime error" not in out, out[-6000:]
    assert r.returncode == 0, out[-6000:]
    assert "crc_check: ok" in out, out[-6000:]


def _count_blocks(path):
    d, o, n = open(path, "rb").read(), 0, 0
    while o < len(d):
        o += int.from_bytes(d[o + 16:o + 18], "little") + 1
        n += 1
    assert o == len(d)
    return n


def test_bgzf_check_good_bam(datadir):
    import grom_amd
    bam, _ = synth(datadir, "three_chr", CASES["three_chr"])
    r = grom_amd.bgzf_check(bam)
    assert r["ok"] and r["failing"] == 0 and r["first_bad"] == -1 and r["bad_off"] == [] and r["error"] is None, r
    assert r["blocks"] == _count_blocks(bam) and r["eof_marker"] is True, r
    assert r["inflated_bytes"] == len(_bgzf.inflated(datadir, "three_chr", CASES["three_chr"]))


def test_bgzf_check_crc_flips_and_missing_eof(datadir, tmp_path):
    import grom_amd
    g = _bgzf.grid_file(datadir)
    info = g["info"]
    good = grom_amd.bgzf_check(g["path"])
    assert good["ok"] and good["blocks"] == len(info) + 1 and good["eof_marker"], good
    assert good["inflated_bytes"] == sum(len(p) for p in g["payloads"])
    i, j = 7, len(info) - 3
    path = str(tmp_path / "flipped.bgzf")

    def edit(p):
        _bgzf.flip_crc_bit(p, info[i], 3)
        _bgzf.flip_crc_bit(p, info[j], 30)
    _bgzf.copy_with(g["path"], path, edit)
    r = grom_amd.bgzf_check(path)
    assert not r["ok"] and r["failing"] == 2 and r["first_bad"] == info[i]["off"], r
    assert r["bad_off"] == [info[i]["off"], info[j]["off"]], r
    assert r["error"] == f"BGZF block at file offset {info[i]['off']} of {path}: CRC-32 mismatch", r
    assert r["blocks"] == good["blocks"] and r["eof_marker"]
    # the good file without its EOF marker: reported, not an error
    path2 = _bgzf.copy_with(g["path"], str(tmp_path / "noeof.bgzf"), _bgzf.drop_eof)
    r = grom_amd.bgzf_check(path2)
    assert r["ok"] and r["eof_marker"] is False and r["blocks"] == good["blocks"] - 1, r
    # a file that ends inside a block is not whole BGZF blocks
    path3 = str(tmp_path / "cut.bgzf")
    with open(path3, "wb") as f:
        f.write(open(g["path"], "rb").read()[:-40])
    with pytest.raises(RuntimeError, match="no whole BGZF block"):
        grom_amd.bgzf_check(path3)


def test_verify_switch_wrapper(monkeypatch):
    import grom_amd
    assert grom_amd.verify_bgzf_crc(True) is None
    assert grom_amd.verify_bgzf_crc(False) is True
    assert grom_amd.verify_bgzf_crc(None) is False
    assert grom_amd.verify_bgzf_crc(None) is None


def _plan_only(sd, bam, env):
    e = {k: v for k, v in os.environ.items() if k != "GROM_VERIFY_CRC"}
    e.update(env, GROM_PLAN_ONLY="1")
    return subprocess.run([GROM_BIN, "-i", bam, "-r", sd["fa"], "-o", "o.vcf"], cwd=os.path.dirname(bam), env=e,
                          capture_output=True, text=True, timeout=300)


def test_silent_damage_host_readers(datadir, monkeypatch):
    """One flipped quality byte in a stored block: the file inflates as before
    and, without the switch, the run ends well (today's behaviour, pinned).
    With GROM_VERIFY_CRC=1 the decoder threads and the serial reader fail and
    name the block; the host index builder fails and leaves no file."""
    import grom_amd
    monkeypatch.delenv("GROM_VERIFY_CRC", raising=False)
    sd = _bgzf.silent_damage(datadir)
    _bgzf.prove_silent(sd)
    want = f"BGZF block at file offset {sd['block_off']} of "
    r = _plan_only(sd, sd["bam"], {})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for env in ({"GROM_VERIFY_CRC": "1"}, {"GROM_VERIFY_CRC": "1", "GROM_SERIAL_DECODE": "1"}):
        r = _plan_only(sd, sd["bam"], env)
        assert r.returncode != 0, (env, r.stdout[-2000:] + r.stderr[-2000:])
        assert want in r.stderr and "CRC-32 mismatch" in r.stderr, (env, r.stderr[-2000:])
        # the undamaged file passes the same check
        r = _plan_only(sd, sd["good"], env)
        assert r.returncode == 0, (env, r.stdout[-2000:] + r.stderr[-2000:])
    # the file check names the same block
    r = grom_amd.bgzf_check(sd["bam"])
    assert r["failing"] == 1 and r["bad_off"] == [sd["block_off"]] and r["blocks"] == sd["blocks"], r
    # the host index builder
    d = datadir / "crc_bai"
    d.mkdir(exist_ok=True)
    bam = str(d / "d.bam")
    shutil.copy(sd["bam"], bam)
    assert grom_amd.lib().grom_bai_build(bam.encode()) == 0
    assert open(bam + ".bai", "rb").read() == open(sd["good"] + ".bai", "rb").read()
    os.remove(bam + ".bai")
    assert grom_amd.verify_bgzf_crc(True) is None
    try:
        assert grom_amd.lib().grom_bai_build(bam.encode()) != 0
        assert want in grom_amd.last_error() and "CRC-32 mismatch" in grom_amd.last_error()
        assert not os.path.exists(bam + ".bai")
        assert grom_amd.lib().grom_bai_build(sd["good"].encode()) == 0  # (the undamaged file, checked: its index again)
    finally:
        grom_amd.verify_bgzf_crc(None)
