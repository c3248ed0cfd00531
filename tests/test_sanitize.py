"""Host code under sanitizers (CPU only): AddressSanitizer + UBSan, and
ThreadSanitizer for the threaded paths.

`make sanitize SAN=asan|tsan` builds tools/san_driver.c against the library's
host sources compiled with the sanitizer (the device objects are linked
uninstrumented and never called) and grom_synth.  The runs cover:
  - the parallel BAM writer (synth.c: generator threads + compression queue,
    libdeflate per-thread compressors) and the BAI it writes (bamio.c);
  - the drop-in CLI with GROM_PLAN_ONLY: BAI planning, the streamed decoder
    (pdecode.c: decoder threads, the in-order uploader, tail sets, insert
    statistics) with small pieces so many borders are crossed, and the serial
    reader (GROM_SERIAL_DECODE);
  - BAI region queries against a linear scan, the SNV row formatter, the
    synthetic-batch builder and the translocation post-pass.
  - the scan worker pool: in plan-only mode the streamed decoder hands every
    chromosome to the pool's threads, which print its plan line;
  - svcall.cpp's candidate lists, SV assembly and rows (sv_rows) on inputs
    recorded from real GPU scans of the "sv" parity case (tests/golden/
    svh_*.svh.gz, written by tools/record_sv_hits.sh with GROM_SV_HITS_DUMP:
    parameters, reference, the per-base hits, every INV depth query with its
    answer, and the rows the GPU run wrote), replayed on concurrent threads,
    four rounds each, and compared with the recorded rows;
  - cnvcall.cpp's CNV host arithmetic on inputs recorded from real GPU scans of
    CNV parity cases whose rows equalled the oracle's (tests/golden/
    cnvh_*.cnvh.gz, written by tools/record_cnv_host.sh with
    GROM_CNV_HOST_DUMP: what the host steps read from the device and every
    result they produced, down to the rows), the records replayed on concurrent
    threads through the samplers, tables, window plan, z override and the
    threaded copy-number step, every recorded output compared byte for byte;
  - the device BGZF inflater's host twin (inflate.h) on the synthetic BAM.
Any sanitizer report fails the test (UBSan is built with
-fno-sanitize-recover, ASan/TSan exit non-zero).
"""
import glob
import gzip
import os
import shutil
import subprocess

import pytest

from _util import REPO

SYNTH_ARGS = ["-L", "300000,200000,150000", "-s", "3", "-c", "12", "-l", "100", "-X", "5", "-V", "1e-5",
              "-W", "2000,20000"]


def _build(san):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    r = subprocess.run(["make", "-s", "sanitize", f"SAN={san}", "-j8"], cwd=REPO, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    d = os.path.join(REPO, "build", f"san-{san}")
    return os.path.join(d, "san_driver"), os.path.join(d, "grom_synth")


def _run(cmd, cwd, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    e.setdefault("ASAN_OPTIONS", "abort_on_error=0:detect_leaks=1")
    e.setdefault("TSAN_OPTIONS", "halt_on_error=1")
    r = subprocess.run(cmd, cwd=cwd, env=e, capture_output=True, text=True, timeout=timeout)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out and "runtime error" not in out, out[-6000:]
    assert r.returncode == 0, out[-6000:]
    return out


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_host_code_under_sanitizer(san, tmp_path):
    driver, synth = _build(san)
    d = str(tmp_path)
    _run([synth, "-o", "s"] + SYNTH_ARGS, d)
    plans = []
    for env in ({}, {"GROM_PIECE_RECS": "1500"}, {"GROM_SERIAL_DECODE": "1"}):
        out = _run([driver, "cli", "-i", "s.bam", "-r", "s.fa", "-o", "o.vcf"], d,
                   dict(env, GROM_PLAN_ONLY="1"))
        plans.append(sorted(line for line in out.splitlines() if line.startswith("plan ")))
    assert len(plans[0]) == 3 and plans[0] == plans[1] == plans[2], plans
    # svcall.cpp on recorded GPU-scan inputs, every record on its own thread
    recs = []
    for gz in sorted(glob.glob(os.path.join(REPO, "tests", "golden", "svh_*.svh.gz"))):
        path = os.path.join(d, os.path.basename(gz)[:-3])
        with gzip.open(gz, "rb") as fi, open(path, "wb") as fo:
            fo.write(fi.read())
        recs.append(path)
    assert len(recs) >= 2
    out = _run([driver, "svrows"] + recs, d)
    assert out.count(": rc 0") == len(recs), out
    # cnvcall.cpp on recorded GPU-scan inputs, every record on its own thread
    recs = []
    for gz in sorted(glob.glob(os.path.join(REPO, "tests", "golden", "cnvh_*.cnvh.gz"))):
        path = os.path.join(d, os.path.basename(gz)[:-3])
        with gzip.open(gz, "rb") as fi, open(path, "wb") as fo:
            fo.write(fi.read())
        recs.append(path)
    assert len(recs) >= 2
    out = _run([driver, "cnvhost"] + recs, d)
    assert out.count(": 0 mismatches") == len(recs), out
    if san == "asan":  # single-threaded helpers: once is enough
        assert "0 mismatches" in _run([driver, "inflate", "s.bam"], d)
        assert "0 mismatches" in _run([driver, "bai", "s.bam", "3000"], d)
        assert "0 mismatches" in _run([driver, "fmt", "20000"], d)
        assert "reads on a" in _run([driver, "synth", "200000"], d)
        assert "rc 0" in _run([driver, "ctx"], d)


# The CLI's GROM_* knobs (cli_settings.c), as `san_driver settings` prints
# them.  This table is the knob reference: field, the variable it reads, what an
# empty environment gives, and what "0", "-5", "1000", "" and "1" give.
_SET, _IS1, _ANY = (1, 1, 1, 1, 1), (0, 0, 0, 0, 1), ("0", "-5", "1000", "", "1")
KNOBS = [
    # set at all
    ("plan_only", "GROM_PLAN_ONLY", 0, _SET), ("verbose", "GROM_VERBOSE", 0, _SET),
    ("fasta_serial", "GROM_FASTA_SERIAL", 0, _SET), ("segv_trace", "GROM_SEGV_TRACE", 0, _SET),
    ("no_warm", "GROM_NO_WARM", 0, _SET), ("stage_digest", "GROM_STAGE_DIGEST", 0, _SET),
    ("copy_stats", "GROM_COPY_STATS", 0, _SET), ("has_seed", "GROM_SEED", 0, _SET),
    ("has_decode_threads", "GROM_DECODE_THREADS", 0, _SET),
    # set to 1
    ("no_ctx_prepare", "GROM_NO_CTX_PREPARE", 0, _IS1), ("par_free", "GROM_PAR_FREE", 0, _IS1),
    ("cli_process", "GROM_CLI_PROCESS", 0, _IS1), ("exit_handlers", "GROM_EXIT_HANDLERS", 0, _IS1),
    ("p_serial", "GROM_P_SERIAL", 0, _IS1),
    ("serial_decode", "GROM_SERIAL_DECODE", 0, (0, 0, 1, 0, 1)),   # above 0
    ("build_index", "GROM_BUILD_INDEX", 0, (0, 1, 1, 0, 1)),       # set and not 0
    # unset (-1), 0 and 1 differ; any other number is neither 0 nor 1
    ("device_decode", "GROM_DEVICE_DECODE", -1, (0, -5, 1000, 0, 1)),
    ("fasta_device", "GROM_FASTA_DEVICE", -1, (0, -5, 1000, 0, 1)),
    # the text as given
    ("dump", "GROM_DUMP", "(unset)", _ANY), ("vcf_segs", "GROM_VCF_SEGS", "(unset)", _ANY),
    ("ctx_raw", "GROM_CTX_RAW", "(unset)", _ANY), ("chroms", "GROM_CHROMS", "(unset)", _ANY),
    ("filedate", "GROM_FILEDATE", "(unset)", _ANY),
    ("seed", "GROM_SEED", 0, (0, 2**32 - 5, 1000, 0, 1)),          # strtoul into 32 bits
    ("device", "GROM_DEVICE", 0, (0, -5, 1000, 0, 1)),
    ("devices", "GROM_DEVICES", 0, (1, 1, 1000, 1, 1)),            # 0: unset; at least 1 (the plan caps it at 64)
    ("scans_per_gpu", "GROM_SCANS_PER_GPU", 2, (1, 1, 1000, 1, 1)),
    ("stages", "GROM_STAGES", 2, (1, 1, 1000, 1, 1)),              # default: the scans per GPU
    ("fasta_threads", "GROM_FASTA_THREADS", 3, (1, 1, 8, 1, 1)),
    # as given: the serial reader takes 4 when unset, the streamed decoder min(CPUs, 32), at least 1
    ("decode_threads", "GROM_DECODE_THREADS", 0, (0, -5, 1000, 0, 1)),
    # unset: -1; an empty list: one worker on the run's device
    ("n_worker_devices", "GROM_WORKER_DEVICES", -1, (1, 1, 1, 0, 1)),
    ("worker_devices", "GROM_WORKER_DEVICES", "", ("0", "-5", "1000", "", "1")),
]


def _settings(driver, env):
    e = {"ASAN_OPTIONS": "abort_on_error=0:detect_leaks=1", "PATH": os.environ.get("PATH", "")}
    e.update(env)
    r = subprocess.run([driver, "settings"], env=e, capture_output=True, text=True, timeout=60)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out and "runtime error" not in out and r.returncode == 0, out[-6000:]
    return dict(line.split("=", 1) for line in r.stdout.splitlines())


def test_cli_settings_under_sanitizer():
    """cli_settings_read, in the stand-alone driver under ASan + UBSan: the
    defaults of an empty environment, the clamps of out-of-range values, every
    knob set to 1, and the three states of the knobs that have three."""
    driver, _ = _build("asan")
    got = _settings(driver, {})
    assert got == {f: str(dflt) for f, _, dflt, _ in KNOBS}, got
    for i, val in enumerate(_ANY):
        got = _settings(driver, {var: val for _, var, _, _ in KNOBS})
        assert got == {f: str(want[i]) for f, _, _, want in KNOBS}, (val, got)
    # a stages default that follows the scans per GPU, and a list of workers
    got = _settings(driver, {"GROM_SCANS_PER_GPU": "3", "GROM_WORKER_DEVICES": "1,0,0"})
    assert (got["scans_per_gpu"], got["stages"]) == ("3", "3")
    assert (got["n_worker_devices"], got["worker_devices"]) == ("3", "1,0,0")
    got = _settings(driver, {"GROM_WORKER_DEVICES": ",".join(["2"] * 70)})
    assert got["n_worker_devices"] == "64"
    for f, var in (("device_decode", "GROM_DEVICE_DECODE"), ("fasta_device", "GROM_FASTA_DEVICE")):
        states = [_settings(driver, env)[f] for env in ({}, {var: "0"}, {var: "1"})]
        assert states == ["-1", "0", "1"], (var, states)
