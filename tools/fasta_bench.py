#!/usr/bin/env python3
"""The device FASTA loader measured on a kept genome.

    python tools/fasta_bench.py --bam G.bam --fasta G.fa --out result.json [--flags -M -g 1]

(a) library level, plain and bgzipped: open (read + upload + inflate), the
    index + length pass, every entry's load -- HIP-event times of the kernels
    and the host clock around each call;
(b) whole CLI runs, alternated, one warm-up and `--runs` timed runs each:
    plain FASTA with the host loader, plain with GROM_FASTA_DEVICE=1, the
    bgzipped FASTA; (c) each run's "candidates/FASTA lengths" phase.
The three variants' rows (the VCF and .ctx.vcf without the ##reference= line)
must hash equal.  The .fa.gz is written beside the output when it is missing
(tools/bgzip_fasta.py's blocks).

    python tools/fasta_bench.py --gzip-leg --fasta G.fa --out gzip.json [--min-mb 256] [--chunks 8 16 32 64]

the plain gzip leg alone: a prefix of the FASTA of at least
--min-mb of text at gzip level 6 (Python's zlib), opened on the device
(GROM_FASTA_GZIP=1) at each chunk size -- stage times by HIP events, the open's
wall time, scratch, units -- beside Python's zlib.decompress of the same file
on this host (one thread) and the BGZF open of the same text."""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

PHASE = re.compile(r"candidates/FASTA lengths ([\d.]+)")


def rows_hash(out):
    h = hashlib.sha256()
    for p in (out, out[:-4] + ".ctx.vcf"):
        for line in open(p, "rb"):
            if not line.startswith(b"##reference="):
                h.update(line)
    return h.hexdigest()[:16]


def library_times(path, device):
    import grom_amd
    t0 = time.perf_counter()
    f = grom_amd.FastaDevice(path, device)
    t1 = time.perf_counter()
    table = f.index()
    t2 = time.perf_counter()
    loads = []
    for i, e in enumerate(table["entries"]):
        before = f.times()
        s = time.perf_counter()
        n = len(f.load(i))
        dt = time.perf_counter() - s
        after = f.times()
        loads.append({"name": e["name"], "bytes": n, "wall_ms": round(dt * 1e3, 2),
                      "kernels_ms": round(after["load_kernels_ms"] - before["load_kernels_ms"], 3),
                      "d2h_ms": round(after["load_d2h_ms"] - before["load_d2h_ms"], 2)})
    times = f.times()
    f.close()
    return {"open_wall_ms": round((t1 - t0) * 1e3, 1), "index_wall_ms": round((t2 - t1) * 1e3, 1),
            "entries": table["n"], "times": {k: round(v, 2) for k, v in times.items()}, "loads": loads}


def gzip_leg(a):
    """The plain gzip read: device open against zlib.decompress on this host."""
    import zlib
    import grom_amd
    from bgzip_fasta import block, PAYLOAD
    work = os.path.abspath(a.work or os.path.dirname(os.path.abspath(a.out)))
    os.makedirs(work, exist_ok=True)
    whole = os.path.getsize(a.fasta)
    with open(a.fasta, "rb") as f:
        text = f.read(min(whole, a.min_mb << 20))
        text += f.readline()  # to a line's end
    res = {"text_bytes": len(text), "whole_fasta_bytes": whole, "input": "whole file" if len(text) >= whole else "prefix"}
    fa, gz, bg = (os.path.join(work, n) for n in ("gzleg.fa", "gzleg.fa.gz", "gzleg.bgzf.fa.gz"))
    with open(fa, "wb") as f:
        f.write(text)
    t0 = time.perf_counter()
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    with open(gz, "wb") as g:
        for o in range(0, len(text), 1 << 24):
            g.write(c.compress(text[o:o + (1 << 24)]))
        g.write(c.flush())
    res["gzip_level"], res["python_compress_s"] = 6, round(time.perf_counter() - t0, 1)
    with open(bg, "wb") as g:
        for o in range(0, len(text), PAYLOAD):
            g.write(block(text[o:o + PAYLOAD], 1))
        g.write(block(b"", 1))
    res["gz_bytes"], res["bgzf_bytes"] = os.path.getsize(gz), os.path.getsize(bg)
    print(json.dumps(res), flush=True)
    # the comparator: what a user does today before bgzip (file in the page cache, one thread)
    zt = []
    for _ in range(3):
        t0 = time.perf_counter()
        with open(gz, "rb") as f:
            out = zlib.decompress(f.read(), 31)
        zt.append(round((time.perf_counter() - t0) * 1e3, 1))
        assert len(out) == len(text)
    del out
    res["zlib_decompress_ms"] = zt
    print(json.dumps({"zlib_decompress_ms": zt}), flush=True)
    os.environ["GROM_FASTA_GZIP"] = "1"

    def opens(path, n=3):
        walls, last = [], None
        for k in range(n + 1):  # the first open warms up (code objects, the page cache)
            t0 = time.perf_counter()
            f = grom_amd.FastaDevice(path, a.device)
            dt = (time.perf_counter() - t0) * 1e3
            last = (f.times(), f.gzip_stats() if f.kind == "gzip" else None)
            f.close()
            if k:
                walls.append(round(dt, 1))
        return walls, last
    res["plain_open_wall_ms"], _ = opens(fa)
    res["bgzf_open_wall_ms"], (bt, _) = opens(bg)
    res["bgzf_inflate_ms"] = round(bt["inflate_ms"], 2)
    res["gzip"] = {}
    for kb in a.chunks:
        os.environ["GROM_GZIP_CHUNK_KB"] = str(kb)
        walls, (tm, st) = opens(gz)
        res["gzip"][str(kb)] = {"open_wall_ms": walls, "read_upload_ms": round(tm["read_upload_ms"], 1),
                                **{k: (round(v, 2) if isinstance(v, float) else v) for k, v in st.items()}}
        print(kb, json.dumps(res["gzip"][str(kb)]), flush=True)
    os.environ.pop("GROM_GZIP_CHUNK_KB", None)
    # one lane's rate: a short prefix with no guesses is one unit (GROM_GZIP_UNIT_MAX_KB sized from this)
    lane = os.path.join(work, "gzleg_lane.fa.gz")
    with open(lane, "wb") as g:
        c = zlib.compressobj(6, zlib.DEFLATED, 31)
        g.write(c.compress(text[:a.lane_mb << 20]) + c.flush())
    os.environ.update(GROM_GZIP_GUESS="0", GROM_GZIP_UNIT_MAX_KB="131072")
    _, (_, st) = opens(lane, 1)
    for k in ("GROM_GZIP_GUESS", "GROM_GZIP_UNIT_MAX_KB"):
        os.environ.pop(k)
    res["one_lane"] = {"text_bytes": a.lane_mb << 20, "gz_bytes": os.path.getsize(lane), "count_ms": round(st["count_ms"], 1),
                       "symbols_ms": round(st["symbols_ms"], 1), "units": st["units"],
                       "compressed_kb_per_s_counting": round(os.path.getsize(lane) / 1.024 / max(st["count_ms"], 1e-9), 1)}
    print(json.dumps(res["one_lane"]), flush=True)
    # the default chunk: the same table as the plain file, and the bar
    with grom_amd.FastaDevice(gz, a.device) as f, grom_amd.FastaDevice(fa, a.device) as g:
        res["index_equal"] = f.index() == g.index()
        n = f.index()["n"]
        res["last_entry_equal"] = f.load(n - 1) == g.load(n - 1)
    walls, _ = opens(gz)
    res["default_open_wall_ms"] = walls
    res["bar"] = {"device_open_ms": min(walls), "zlib_ms": min(zt), "ratio": round(min(zt) / min(walls), 2),
                  "met": 2 * min(walls) <= min(zt)}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["bar"]), "index equal:", res["index_equal"], res["last_entry_equal"])
    return 0 if res["index_equal"] and res["last_entry_equal"] else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--gzip-leg", action="store_true", help="the plain gzip leg alone (no BAM needed)")
    ap.add_argument("--min-mb", type=int, default=256)
    ap.add_argument("--lane-mb", type=int, default=2, help="text of the one-lane rate probe")
    ap.add_argument("--chunks", type=float, nargs="*", default=[8, 16, 32, 64, 128])
    ap.add_argument("--bam", default="")
    ap.add_argument("--fasta", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--work", default="")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--flags", nargs=argparse.REMAINDER, default=[])
    a = ap.parse_args()
    if a.gzip_leg:
        return gzip_leg(a)
    if not a.bam:
        ap.error("--bam is required")
    import grom_amd
    from bgzip_fasta import block, PAYLOAD
    work = os.path.abspath(a.work or os.path.dirname(os.path.abspath(a.out)))
    a.out = os.path.abspath(a.out)
    os.makedirs(work, exist_ok=True)
    for src, name in ((a.bam, "g.bam"), (a.bam + ".bai", "g.bam.bai"), (a.fasta, "g.fa")):
        dst = os.path.join(work, name)
        if not os.path.exists(dst):
            os.symlink(os.path.abspath(src), dst)
    gz = os.path.join(work, "g.fa.gz")
    res = {}
    if not os.path.exists(gz):
        t0 = time.perf_counter()
        with open(a.fasta, "rb") as f, open(gz, "wb") as g:
            while True:
                p = f.read(PAYLOAD)
                if not p:
                    break
                g.write(block(p, 1))
            g.write(block(b"", 1))
        res["bgzip_s"] = round(time.perf_counter() - t0, 1)
    res["fasta_bytes"], res["fasta_gz_bytes"] = os.path.getsize(a.fasta), os.path.getsize(gz)
    res["library"] = {"plain": library_times(os.path.join(work, "g.fa"), a.device), "bgzf": library_times(gz, a.device)}
    print(json.dumps(res["library"]), flush=True)
    variants = {"plain_host": ("g.fa", {}), "plain_device": ("g.fa", {"GROM_FASTA_DEVICE": "1"}), "bgzf_device": ("g.fa.gz", {})}
    env0 = dict(os.environ, GROM_FILEDATE="20260101", GROM_SEED="7", GROM_VERBOSE="1")
    runs = {v: [] for v in variants}
    hashes = {}
    for k in range(a.runs + 1):  # round 0 warms each variant up (and writes its .info)
        for v, (fa, extra) in variants.items():
            out = os.path.join(work, f"{v}.vcf")
            t0 = time.perf_counter()
            r = subprocess.run([grom_amd.GROM_BIN, "-i", "g.bam", "-r", fa, "-o", out] + a.flags, cwd=work,
                               env=dict(env0, **extra), capture_output=True, text=True, timeout=900)
            dt = time.perf_counter() - t0
            if r.returncode != 0:
                raise SystemExit(f"{v}: grom failed ({r.returncode}): {r.stdout[-2000:]} {r.stderr[-2000:]}")
            m = PHASE.search(r.stdout)
            loader = [l for l in r.stderr.splitlines() if "device FASTA loader" in l]
            hashes.setdefault(v, set()).add(rows_hash(out))
            if k > 0:
                runs[v].append({"wall_s": round(dt, 3), "fasta_lengths_phase_s": float(m.group(1)) if m else None,
                                "loader": loader[-1] if loader else None})
            print(v, k, round(dt, 3), m.group(1) if m else "-", flush=True)
    res["cli"] = runs
    res["rows_hash"] = {v: sorted(h) for v, h in hashes.items()}
    res["rows_equal"] = len(set().union(*hashes.values())) == 1
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("rows equal:", res["rows_equal"])
    return 0 if res["rows_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
