"""The reference FASTA read on the device, bgzip-compressed or plain
(grom_fasta_dev_*, fastadev.hip): its index and loads are the host code's
(grom_fasta_open / grom_fasta_load, stream.c), bit for bit.

One edge-case file of about 80 kB is written here (zlib and struct only, as
test_bai_device.py writes BGZF): text before the first header, 60-column lines
with a short last line, CRLF endings, an empty entry, a blank line inside an
entry, a line of its predecessor's length ending in `**` (the predecessor's
cut is kept), a line starting with digits, a 2,500-byte and a 70,000-byte line
(999-byte chunks crossing 64 KB block ends), a header longer than 999 bytes, a
long line whose second 999-byte chunk begins with `>` (an entry on both
sides), an all-N stretch, lower-case bases, a name over 49 bytes and a last
line with no newline.  It is written plain and as BGZF with payload sizes
cycling through 997, 1, 4093, 65280 and 37 bytes, an empty block in the
middle, the EOF block last, at levels 0, 1 and 9 and with Z_FIXED."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import zlib

import pytest

from _util import CASES, GROM_BIN, TILAPIA_FA, run_grom, run_oracle, synth

PAYLOADS = (997, 1, 4093, 65280, 37)
VARIANTS = {"l1": (1, zlib.Z_DEFAULT_STRATEGY), "l0": (0, zlib.Z_DEFAULT_STRATEGY), "l9": (9, zlib.Z_DEFAULT_STRATEGY),
            "fixed": (6, zlib.Z_FIXED)}
_cache = {}


def _block(payload, level=1, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    z = c.compress(payload) + c.flush()
    assert len(z) + 26 <= 65536
    return (struct.pack("<4BI2BH2B2H", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(z) + 25) + z +
            struct.pack("<II", zlib.crc32(payload), len(payload)))


def write_bgzf(data, path, level=1, strategy=zlib.Z_DEFAULT_STRATEGY, payloads=PAYLOADS):
    blocks, o, k = [], 0, 0
    while o < len(data):
        n = payloads[k % len(payloads)]
        blocks.append(_block(data[o:o + n], level, strategy))
        o += n
        k += 1
        if k == 7:
            blocks.append(_block(b"", level, strategy))  # an empty block in the middle
    blocks.append(_block(b""))  # the EOF block
    with open(path, "wb") as f:
        f.write(b"".join(blocks))


def _bases(n, seed):
    out, x = bytearray(), seed * 2654435761 % (1 << 32) or 1
    for _ in range(n):
        x = (x * 1103515245 + 12345) % (1 << 31)
        out.append(b"ACGT"[(x >> 16) & 3])
    return bytes(out)


def _lines(seq, w=60, eol=b"\n"):
    return b"".join(seq[i:i + w] + eol for i in range(0, len(seq), w))


def edge_text():
    t = [b"ACGTNNacgtnn\nTTTTGGGG\n"]                                  # text before the first header
    t += [b">chr1 the first entry\n", _lines(_bases(60 * 40 + 23, 1))]   # 60 columns, a short last line
    t += [b">crlf\r\n", _lines(_bases(60 * 12 + 7, 2), eol=b"\r\n")]     # CRLF line endings
    t += [b">empty\n", b">after_empty\tx\n", _lines(_bases(60 * 3, 3))]  # a header directly after a header
    t += [b"\n", _lines(_bases(60 * 2 + 5, 4))]                          # a blank line inside the entry
    t += [b">stars\n", _bases(60, 5) + b"\n", _bases(58, 6) + b"**\n",   # same length, ends in ** (cut kept)
          _bases(60, 7) + b"\n", b"12345" + _bases(40, 8) + b"\n",       # a line that starts with digits
          b"123\n", b"**\n", _bases(30, 9) + b"\n"]
    t += [b">long2500\n", _bases(2500, 10) + b"\n", _lines(_bases(130, 11))]
    t += [b">long70000\n", _bases(70000, 12) + b"\n", _lines(_bases(61, 13))]
    t += [b">longheader " + b"h" * 1200 + b" tail\n", _lines(_bases(200, 14))]  # a header longer than 999 bytes
    t += [b">split\n", _bases(999, 15) + b">mid in a long line " + _bases(700, 16) + b"\n", _lines(_bases(90, 17))]
    t += [b">masked\n", _lines(b"N" * 400 + _bases(200, 18).lower() + b"n" * 77 + _bases(100, 19))]
    t += [b">" + b"a_name_that_is_longer_than_the_forty_nine_bytes_kept_Z" + b" d\n", _lines(_bases(150, 20))]
    t += [b">Last_ONE\n", _lines(_bases(120, 21)), _bases(33, 22)]       # no newline at the end of the file
    return b"".join(t)


def files(datadir):
    """The edge-case file, plain and in every BGZF variant (written once)."""
    if "files" not in _cache:
        d = os.path.join(str(datadir), "fasta_device")
        os.makedirs(d, exist_ok=True)
        text = edge_text()
        assert 75000 < len(text) < 90000
        paths = {"plain": os.path.join(d, "edge.fa")}
        with open(paths["plain"], "wb") as f:
            f.write(text)
        for v, (level, strategy) in VARIANTS.items():
            paths[v] = os.path.join(d, f"edge_{v}.fa.gz")
            write_bgzf(text, paths[v], level, strategy)
        _cache["files"] = (text, paths)
    return _cache["files"]


# ---- the rule, restated (ISSUE / DESIGN.md 4.7) ----
def _alpha(c):
    return 65 <= c <= 90 or 97 <= c <= 122


def _chunks(data, start):
    """fgets(line, 1000) from `start`: a chunk ends after its newline, at 999 bytes or at the end."""
    q = start
    while q < len(data):
        nl = data.find(b"\n", q, q + 999)
        e = nl + 1 if nl >= 0 else min(q + 999, len(data))
        yield q, e
        q = e


def py_index(data):
    ent, mappable = [], 0
    for q, e in _chunks(data, 0):
        c = data[q:e]
        if c[:1] == b">":
            name_end = len(c)
            for w in range(len(c) - 1, 0, -1):
                if not 33 <= c[w] <= 126:
                    name_end = w
            name_end = min(name_end, 50)
            ent.append({"name": c[1:name_end].decode("latin-1").lower(), "name_len": name_end - 1, "file_pos": e,
                        "len": 0})
        else:
            a = sum(1 for x in c if _alpha(x))
            mappable += sum(1 for x in c if _alpha(x) and x not in b"Nn")
            if ent:
                ent[-1]["len"] += a
    return {"n": len(ent), "mappable": mappable, "entries": ent}


def py_load(data, file_pos):
    out, prev_l, alpha = [], -1, 0
    for q, e in _chunks(data, file_pos):
        c = data[q:e]
        if c[:1] == b">":
            break
        if not out or len(c) != prev_l:
            prev_l = len(c)
            w = len(c) - 1
            while w > 0 and not _alpha(c[w]):
                w -= 1
            alpha = w + 1
        out.append(c[:alpha])
    return b"".join(out)


def _strip(table):
    """The fields the host table has (the device adds load_len)."""
    return {"n": table["n"], "mappable": table["mappable"],
            "entries": [{k: e[k] for k in ("name", "name_len", "file_pos", "len")} for e in table["entries"]]}


def host_all(path):
    """The host's table and every entry's bytes (computed once per file)."""
    import grom_amd
    key = ("host", path)
    if key not in _cache:
        t = grom_amd.fasta_index(path)
        _cache[key] = (t, [grom_amd.fasta_load(path, i) for i in range(t["n"])])
    return _cache[key]


def _info_text(plain_fa):
    """<fasta>.info (save_genome_info's format) of the host's table of the plain file."""
    import grom_amd
    t = grom_amd.fasta_index(plain_fa)
    return f"{t['n']} {t['mappable']}\n" + "".join(
        f"{i} {e['name_len']} {e['file_pos']} {e['len']} {e['name']}\n" for i, e in enumerate(t["entries"]))


# ---- CPU ----
def test_rule_restated_agrees_with_host(datadir):
    text, paths = files(datadir)
    want = py_index(text)
    assert want["n"] == 13
    table, loads = host_all(paths["plain"])
    assert table == want
    names = [e["name"] for e in table["entries"]]
    assert names[:5] == ["chr1", "crlf", "empty", "after_empty", "stars"] and "mid" in names and names[-1] == "last_one"
    assert table["entries"][-2]["name_len"] == 49 and len(loads[2]) == 0
    for e, got in zip(table["entries"], loads):
        assert got == py_load(text, e["file_pos"]), e["name"]
    # the kept cut: `**` of the line with its predecessor's length stays in the reference
    assert b"**" in loads[names.index("stars")]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_bgzf_through_the_host_path(datadir, variant):
    text, paths = files(datadir)
    assert host_all(paths[variant]) == host_all(paths["plain"])


def test_gzip_that_is_not_bgzf_is_refused(datadir, tmp_path):
    import gzip
    import grom_amd
    text, _ = files(datadir)
    p = str(tmp_path / "plain_gzip.fa.gz")
    with gzip.open(p, "wb") as f:
        f.write(text)
    with pytest.raises(RuntimeError):
        grom_amd.fasta_index(p)
    assert "recompress it with bgzip" in grom_amd.last_error()
    bam0, _ = synth(datadir, "one_chr", CASES["one_chr"])
    shutil.copy(bam0, str(tmp_path / "y.bam"))
    shutil.copy(bam0 + ".bai", str(tmp_path / "y.bam.bai"))
    r = subprocess.run([GROM_BIN, "-i", "y.bam", "-r", "plain_gzip.fa.gz", "-o", "y.vcf"], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "recompress it with bgzip" in r.stdout + r.stderr


def test_info_of_a_bgzf_file_loads_back(datadir, tmp_path):
    """<fasta>.info written for the .fa.gz (the CLI's open, host path) holds the
    plain file's table: file_pos are offsets in the inflated text."""
    bam0, fa0 = synth(datadir, "three_chr", CASES["three_chr"])
    write_bgzf(open(fa0, "rb").read(), str(tmp_path / "r.fa.gz"))
    for n in ("", ".bai"):
        shutil.copy(bam0 + n, str(tmp_path / ("r.bam" + n)))
    env = dict(os.environ, GROM_PLAN_ONLY="1", GROM_FASTA_DEVICE="0")
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


# ---- GPU ----
def _device_equals_host(path, ref_path):
    import grom_amd
    table, loads = host_all(ref_path)
    with grom_amd.FastaDevice(path, 0) as f:
        got = f.index()
        assert _strip(got) == table
        assert [e["load_len"] for e in got["entries"]] == [len(b) for b in loads]
        for i, want in enumerate(loads):
            assert f.load(i) == want, table["entries"][i]["name"]
    # a table adopted from outside (the .info path): lengths measured by the loads
    with grom_amd.FastaDevice(path, 0) as f:
        f.set_index(table)
        for i in (len(loads) - 1, 0, 2, 7):
            assert f.load_len(i) == len(loads[i])
            assert f.load(i) == loads[i]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain"] + list(VARIANTS))
def test_edge_file_device_equals_host(datadir, variant):
    _, paths = files(datadir)
    _device_equals_host(paths[variant], paths["plain"])


@pytest.mark.gpu
@pytest.mark.parametrize("variant,piece_kb", [("plain", "4"), ("l1", "4"), ("l9", "7.3")])
def test_small_pieces(datadir, monkeypatch, variant, piece_kb):
    """Entries and long lines straddle the pieces of the scans (and the inflate launches)."""
    monkeypatch.setenv("GROM_FASTA_PIECE_KB", piece_kb)
    _, paths = files(datadir)
    _device_equals_host(paths[variant], paths["plain"])


@pytest.mark.gpu
def test_nul_byte_is_host_only(datadir, tmp_path):
    import grom_amd
    text, _ = files(datadir)
    at = text.index(b">long2500") + 1500
    bad = text[:at] + b"\0" + text[at + 1:]
    for name, write in (("nul.fa", lambda p: open(p, "wb").write(bad)), ("nul.fa.gz", lambda p: write_bgzf(bad, p))):
        p = str(tmp_path / name)
        write(p)
        with pytest.raises(grom_amd.FastaHostOnly):
            grom_amd.fasta_index(p, 0)
        table = grom_amd.fasta_index(p)
        i = [e["name"] for e in table["entries"]].index("long2500")
        with grom_amd.FastaDevice(p, 0) as f:
            f.set_index(table)
            with pytest.raises(grom_amd.FastaHostOnly):
                f.load(i)
            assert f.load(0) == grom_amd.fasta_load(p, 0)  # an entry without the byte still loads
        # the load as the CLI does it: the host path when the device says so
        assert grom_amd.fasta_load(p, i, device=0) == grom_amd.fasta_load(p, i)


@pytest.mark.gpu
def test_tilapia_contig_as_bgzf(datadir, tmp_path):
    import grom_amd
    p = str(tmp_path / "tilapia.fa.gz")
    write_bgzf(open(TILAPIA_FA, "rb").read(), p, payloads=(65280,))
    table, loads = host_all(TILAPIA_FA)
    with grom_amd.FastaDevice(p, 0) as f:
        assert f.bgzf
        got = f.index()
        assert _strip(got) == table
        for i, want in enumerate(loads):
            assert got["entries"][i]["load_len"] == len(want)
            assert f.load(i) == want


def _cli_case(datadir, tmp_path, case):
    bam0, fa0 = synth(datadir, case, CASES[case])
    for n in ("", ".bai"):
        shutil.copy(bam0 + n, str(tmp_path / (case + ".bam" + n)))
    shutil.copy(fa0, str(tmp_path / (case + ".fa")))
    write_bgzf(open(fa0, "rb").read(), str(tmp_path / (case + ".fa.gz")))
    return case + ".bam", case + ".fa", case + ".fa.gz"


def _read(p, skip_reference=False):
    lines = open(str(p)).read().splitlines(True)
    return [l for l in lines if not (skip_reference and l.startswith("##reference="))]


@pytest.mark.gpu
def test_cli_three_chr_bgzf_and_plain_on_the_device(datadir, tmp_path, capfd):
    bam, fa, gz = _cli_case(datadir, tmp_path, "three_chr")
    run_oracle(tmp_path, bam, fa, "o.vcf")
    flush = C.CDLL(None).fflush  # the CLI runs in this process: its stdio buffers
    capfd.readouterr()
    run_grom(tmp_path, bam, gz, "g.vcf", env_extra={"GROM_VERBOSE": "1"})
    flush(None)
    err = capfd.readouterr().err
    assert "device FASTA loader" in err and "BGZF" in err
    for ext in (".vcf", ".ctx.vcf"):
        assert _read(tmp_path / ("g" + ext), True) == _read(tmp_path / ("o" + ext), True)
    assert "##reference=three_chr.fa.gz\n" in _read(tmp_path / "g.vcf")
    # the .info written for the .fa.gz is the plain file's (uncompressed offsets); a second run adopts it
    assert open(str(tmp_path / (gz + ".info"))).read() == _info_text(str(tmp_path / fa))
    run_grom(tmp_path, bam, gz, "g2.vcf")
    for ext in (".vcf", ".ctx.vcf"):
        assert _read(tmp_path / ("g2" + ext)) == _read(tmp_path / ("g" + ext))
    # the plain file through the device loader: the oracle's bytes, header included
    capfd.readouterr()
    run_grom(tmp_path, bam, fa, "p.vcf", env_extra={"GROM_VERBOSE": "1", "GROM_FASTA_DEVICE": "1"})
    flush(None)
    assert "device FASTA loader" in capfd.readouterr().err
    for ext in (".vcf", ".ctx.vcf"):
        assert _read(tmp_path / ("p" + ext)) == _read(tmp_path / ("o" + ext))


@pytest.mark.gpu
def test_cli_sv_tab_rows_with_bgzf(datadir, tmp_path):
    bam, fa, gz = _cli_case(datadir, tmp_path, "sv")
    run_oracle(tmp_path, bam, fa, "o.txt", ["-f"])
    run_grom(tmp_path, bam, gz, "g.txt", ["-f"])
    assert _read(tmp_path / "g.txt") == _read(tmp_path / "o.txt")
    assert _read(tmp_path / "g.txt.ctx") == _read(tmp_path / "o.txt.ctx")
