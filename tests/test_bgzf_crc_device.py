"""BGZF block checksums on the GPU (k_bgzf_crc, ddecode.hip): the file check
against its host twin on the length grid, and GROM_VERIFY_CRC=1 on every
device path that inflates BGZF -- the BAM decode, the index builder, the BGZF
FASTA open -- with damage that inflates to the right length.  The files are
the generated cases the other tests cache and files of a few hundred KB
written by tests/_bgzf.py."""
import os
import shutil
import subprocess

import pytest

import _bgzf
from _util import CASES, FILEDATE, GROM_BIN, SEED, run_grom, synth

pytestmark = pytest.mark.gpu

SAME = ("blocks", "failing", "first_bad", "inflated_bytes", "eof_marker", "ok", "bad_off")


def _subset(info):
    """The first block, the last data block, an empty block, a 1-byte block, a 65280-byte block and two more."""
    n = [b["n"] for b in info]
    s = {0, len(info) - 1, n.index(0), n.index(1), n.index(65280), n.index(1008), len(n) - 1 - n[::-1].index(65279)}
    return sorted(s)


def _flipped(g, tmp_path, name):
    info, s = g["info"], _subset(g["info"])

    def edit(p):
        for k, i in enumerate(s):
            _bgzf.flip_crc_bit(p, info[i], (5 * k + 1) % 32)
    return _bgzf.copy_with(g["path"], str(tmp_path / name), edit), [info[i]["off"] for i in s]


def test_grid_file_device_equals_host(datadir, tmp_path, monkeypatch):
    import grom_amd
    monkeypatch.delenv("GROM_CHECK_PIECE_KB", raising=False)
    g = _bgzf.grid_file(datadir)
    offs, o = [], 0
    for p in g["payloads"]:
        offs.append(o % 16)
        o += len(p)
    assert set(offs) == set(range(16))  # every start alignment of a block in the inflated piece
    host, dev = grom_amd.bgzf_check(g["path"]), grom_amd.bgzf_check(g["path"], device=0)
    assert dev["ok"] and dev["pieces"] == 1 and dev["device_us"] > 0, dev
    assert {k: dev[k] for k in SAME} == {k: host[k] for k in SAME}, (dev, host)
    assert dev["blocks"] == len(g["info"]) + 1 and dev["eof_marker"]
    path, want = _flipped(g, tmp_path, "flipped.bgzf")
    host, dev = grom_amd.bgzf_check(path), grom_amd.bgzf_check(path, device=0)
    assert not dev["ok"] and dev["bad_off"] == want == host["bad_off"], (dev, host, want)
    assert {k: dev[k] for k in SAME} == {k: host[k] for k in SAME}
    assert dev["error"] == f"BGZF block at file offset {want[0]} of {path}: CRC-32 mismatch"
    # without the EOF marker: reported, not an error
    p2 = _bgzf.copy_with(g["path"], str(tmp_path / "noeof.bgzf"), _bgzf.drop_eof)
    dev = grom_amd.bgzf_check(p2, device=0)
    assert dev["ok"] and dev["eof_marker"] is False and dev["blocks"] == len(g["info"]), dev
    # a file that ends inside a block
    p3 = str(tmp_path / "cut.bgzf")
    with open(p3, "wb") as f:
        f.write(open(g["path"], "rb").read()[:-40])
    with pytest.raises(RuntimeError, match="no whole BGZF block"):
        grom_amd.bgzf_check(p3, device=0)


def test_grid_file_small_pieces(datadir, tmp_path, monkeypatch):
    """Pieces of 64 KB of inflated bytes: many pieces, each ending where a
    block ends (the 65279- and 65280-byte blocks are pieces of their own, and
    the blocks after them the first of the next piece), damaged blocks that
    are first in their piece (the flipped 65280-byte block) and last."""
    import grom_amd
    g = _bgzf.grid_file(datadir)
    path, want = _flipped(g, tmp_path, "flipped.bgzf")
    monkeypatch.delenv("GROM_CHECK_PIECE_KB", raising=False)
    whole_good, whole_bad = grom_amd.bgzf_check(g["path"], device=0), grom_amd.bgzf_check(path, device=0)
    monkeypatch.setenv("GROM_CHECK_PIECE_KB", "64")
    good, bad = grom_amd.bgzf_check(g["path"], device=0), grom_amd.bgzf_check(path, device=0)
    assert good["pieces"] > 10 and bad["pieces"] == good["pieces"], (good, bad)
    assert {k: good[k] for k in SAME} == {k: whole_good[k] for k in SAME} and good["ok"]
    assert {k: bad[k] for k in SAME} == {k: whole_bad[k] for k in SAME} and bad["bad_off"] == want


def _cli(sd, bam, env):
    e = {k: v for k, v in os.environ.items() if k != "GROM_VERIFY_CRC"}
    e.update(env, GROM_FILEDATE=FILEDATE, GROM_SEED=SEED, GROM_DEVICE_DECODE="1")
    return subprocess.run([GROM_BIN, "-i", bam, "-r", sd["fa"], "-o", "o.vcf"], cwd=os.path.dirname(bam), env=e,
                          capture_output=True, text=True, timeout=300)


def test_cli_device_decode_silent_damage(datadir):
    """One flipped quality byte in a stored block of three_chr: without the
    switch the device decode runs to the end; with it every mode stops with
    the block's offset.  Each mode runs once."""
    sd = _bgzf.silent_damage(datadir)
    _bgzf.prove_silent(sd)
    r = _cli(sd, sd["bam"], {"GROM_VERBOSE": "1"})
    assert r.returncode == 0 and "device decode:" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "block checksums" not in r.stdout
    want = f"BGZF block at file offset {sd['block_off']} of "
    for env in ({}, {"GROM_DD_PIECE_MB": "0.0625"}, {"GROM_DD_WORKERS": "2"}):
        r = _cli(sd, sd["bam"], dict(env, GROM_VERIFY_CRC="1"))
        assert r.returncode != 0, (env, r.stdout[-2000:] + r.stderr[-2000:])
        assert want in r.stderr and "CRC-32 mismatch" in r.stderr, (env, r.stderr[-3000:])
        assert "reading the BAM serially" not in r.stdout  # (no other reader is tried)


@pytest.mark.parametrize("case", ["three_chr", "sv"])
def test_undamaged_outputs_identical_with_the_switch(datadir, capfd, case):
    bam, fa = synth(datadir, case, CASES[case])
    run_grom(datadir, bam, fa, f"crc_off_{case}.vcf", env_extra={"GROM_DEVICE_DECODE": "1"})
    capfd.readouterr()
    run_grom(datadir, bam, fa, f"crc_on_{case}.vcf",
             env_extra={"GROM_DEVICE_DECODE": "1", "GROM_VERIFY_CRC": "1", "GROM_VERBOSE": "1"})
    out = capfd.readouterr().out
    assert "block checksums: every BGZF block's CRC-32 checked on the GPU" in out, out[-2000:]
    for ext in (".vcf", ".ctx.vcf"):
        assert open(datadir / f"crc_on_{case}{ext}", "rb").read() == open(datadir / f"crc_off_{case}{ext}", "rb").read()


def test_index_builder_silent_damage(datadir, tmp_path):
    import grom_amd
    sd = _bgzf.silent_damage(datadir)
    bam = str(tmp_path / "d.bam")
    shutil.copy(sd["bam"], bam)
    # the switch off: the host builder's bytes, as today
    assert grom_amd.verify_bgzf_crc(False) is None
    try:
        grom_amd.bai_build(bam)
        assert open(bam + ".bai", "rb").read() == open(sd["good"] + ".bai", "rb").read()
        os.remove(bam + ".bai")
        grom_amd.verify_bgzf_crc(True)
        with pytest.raises(RuntimeError, match=f"BGZF block at file offset {sd['block_off']} of .*CRC-32 mismatch"):
            grom_amd.bai_build(bam)
        assert sorted(os.listdir(tmp_path)) == ["d.bam"]  # neither an index nor a temporary file
        # the undamaged file, checked: the same index
        good = str(tmp_path / "g.bam")
        shutil.copy(sd["good"], good)
        grom_amd.bai_build(good)
        assert open(good + ".bai", "rb").read() == open(sd["good"] + ".bai", "rb").read()
    finally:
        grom_amd.verify_bgzf_crc(None)


def test_bgzf_fasta_stored_crc_flip(datadir, tmp_path):
    import grom_amd
    bam0, fa0 = synth(datadir, "three_chr", CASES["three_chr"])
    text = open(fa0, "rb").read()
    payloads = [text[k:k + 20000] for k in range(0, len(text), 20000)]
    gz = str(tmp_path / "r.fa.gz")
    info = _bgzf.write_bgzf(gz, payloads, stored={2})
    for n in ("", ".bai"):
        shutil.copy(bam0 + n, str(tmp_path / ("r.bam" + n)))
    with grom_amd.FastaDevice(gz, 0) as f:  # (undamaged: the table, switch off and on)
        table = f.index()
    assert grom_amd.verify_bgzf_crc(True) is None
    try:
        with grom_amd.FastaDevice(gz, 0) as f:
            assert f.index() == table
        k = len(info) // 2
        _bgzf.flip_crc_bit(gz, info[k], 9)
        with pytest.raises(RuntimeError, match=f"BGZF block at file offset {info[k]['off']} of .*CRC-32 mismatch"):
            grom_amd.FastaDevice(gz, 0)
        grom_amd.verify_bgzf_crc(False)
        with grom_amd.FastaDevice(gz, 0) as f:  # the switch off: it loads as today
            assert f.index() == table
    finally:
        grom_amd.verify_bgzf_crc(None)
    # the CLI does not recover through the host reader
    e = {k: v for k, v in os.environ.items() if k != "GROM_VERIFY_CRC"}
    e.update(GROM_FILEDATE=FILEDATE, GROM_SEED=SEED)
    r = subprocess.run([GROM_BIN, "-i", "r.bam", "-r", "r.fa.gz", "-o", "off.vcf"], cwd=str(tmp_path), env=e,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([GROM_BIN, "-i", "r.bam", "-r", "r.fa.gz", "-o", "on.vcf"], cwd=str(tmp_path),
                       env=dict(e, GROM_VERIFY_CRC="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"BGZF block at file offset {info[k]['off']} of " in r.stderr + r.stdout, r.stderr[-3000:]
