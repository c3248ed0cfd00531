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
(tools/bgzip_fasta.py's blocks)."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--bam", required=True)
    ap.add_argument("--fasta", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--work", default="")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--flags", nargs=argparse.REMAINDER, default=[])
    a = ap.parse_args()
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
