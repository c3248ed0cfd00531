"""CPU checks of the CNV oracle's restatements of the C library behaviour the
reference's static binary links, pinned against this
host's glibc: rand() after srand() (TYPE_3 additive feedback, unchanged since
glibc 2.0, so also glibc 2.12's) and qsort (merge sort in glibc < 2.37), and a
seed-determinism check of the oracle's CNV rows.  The library's own copies of
these primitives (cnvcall.cpp: GlibcRand, msort_lo, the three bisects shared
with the kernels) are pinned the same way, the bisects against the oracle's."""
import ctypes
import os

import numpy as np
import pytest

from _util import CASES, ORACLE_LIB, run_oracle, synth

libc = ctypes.CDLL("libc.so.6")
libc.rand.restype = ctypes.c_int
libc.srand.argtypes = [ctypes.c_uint]


def oracle():
    lib = ctypes.CDLL(ORACLE_LIB)
    lib.grom_oracle_rand_seq.argtypes = [ctypes.c_uint, ctypes.c_int, ctypes.c_void_p]
    lib.grom_oracle_msort_lo.argtypes = [ctypes.c_void_p, ctypes.c_long]
    lib.grom_oracle_grom_rand.argtypes = [ctypes.c_uint, ctypes.c_long, ctypes.c_int, ctypes.c_void_p]
    return lib


@pytest.mark.parametrize("seed", [0, 1, 7, 1792129490, 4294967295])
def test_rand_matches_glibc(seed):
    n = 5000
    out = np.zeros(n, np.int32)
    oracle().grom_oracle_rand_seq(seed, n, out.ctypes.data)
    libc.srand(seed)
    ref = np.array([libc.rand() for _ in range(n)], np.int32)
    assert np.array_equal(out, ref)


def test_grom_rand_digitwise_bounds():
    """grom_rand(max) (GROM.c:1185-1201) draws decimal digits below max."""
    out = np.zeros(2000, np.int64)
    oracle().grom_oracle_grom_rand(11, 123457, 2000, out.ctypes.data)
    assert out.min() >= 0 and out.max() < 123457
    assert len(np.unique(out)) > 1500


CMP = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)


@CMP
def _cmp_lo(a, b):
    """cmpfunc (GROM.c:1105) applied to doubles: int subtraction of the low words."""
    x = ctypes.c_uint32.from_address(a).value
    y = ctypes.c_uint32.from_address(b).value
    return ctypes.c_int32((x - y) & 0xffffffff).value


@pytest.mark.skipif(tuple(int(v) for v in os.confstr("CS_GNU_LIBC_VERSION").split()[1].split(".")[:2]) >= (2, 37),
                    reason="glibc >= 2.37 replaced the merge sort")
@pytest.mark.parametrize("n", [1, 2, 17, 1000, 40000])
def test_msort_matches_glibc_qsort(n):
    rng = np.random.default_rng(n)
    a = (rng.integers(0, 60, n) / rng.uniform(10, 40)).astype(np.float64)  # ratios like rd / ave
    b = a.copy()
    oracle().grom_oracle_msort_lo(a.ctypes.data, n)
    libc.qsort(b.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(n), ctypes.c_size_t(8), _cmp_lo)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def library():
    """cnvcall.cpp's exported test hooks (host code: no device is touched)."""
    import grom_amd
    lib = grom_amd.lib()
    lib.grom_cnv_test_rand.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
    lib.grom_cnv_test_rand.restype = None
    lib.grom_cnv_test_msort_lo.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    lib.grom_cnv_test_msort_lo.restype = None
    lib.grom_cnv_test_bisect.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_double]
    lib.grom_cnv_test_bisect.restype = ctypes.c_long
    return lib


@pytest.mark.parametrize("seed", [0, 1, 7, 1792129490, 4294967295])
def test_library_rand_matches_glibc(seed):
    n = 5000
    out = np.zeros(n, np.int32)
    library().grom_cnv_test_rand(seed, n, out.ctypes.data)
    libc.srand(seed)
    ref = np.array([libc.rand() for _ in range(n)], np.int32)
    assert np.array_equal(out, ref)


@pytest.mark.skipif(tuple(int(v) for v in os.confstr("CS_GNU_LIBC_VERSION").split()[1].split(".")[:2]) >= (2, 37),
                    reason="glibc >= 2.37 replaced the merge sort")
@pytest.mark.parametrize("n", [1, 2, 17, 1000, 40000])
def test_library_msort_matches_glibc_qsort(n):
    rng = np.random.default_rng(n)
    a = (rng.integers(0, 60, n) / rng.uniform(10, 40)).astype(np.float64)  # ratios like rd / ave
    b = a.copy()
    library().grom_cnv_test_msort_lo(a.ctypes.data, n)
    libc.qsort(b.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(n), ctypes.c_size_t(8), _cmp_lo)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("n", [0, 1, 2, 3, 1000])
def test_library_bisects_match_the_oracle(n):
    """The bisects the kernels and cnvcall.cpp share (cnv_bisect.h) against the
    oracle's on sorted lists with duplicates, probed below, inside and above
    the range: the off-by-one exits of GROM.c:21630-21860 are the point."""
    orc = ctypes.CDLL(ORACLE_LIB)
    orc.grom_oracle_bisect.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_double]
    orc.grom_oracle_bisect.restype = ctypes.c_long
    lib = library()
    rng = np.random.default_rng(100 + n)
    # (one spare entry: both sides read l[0] of an empty list and ignore it)
    li = np.zeros(n + 1, np.int32)
    li[:n] = np.sort(rng.integers(5, 5 + max(n // 3, 2), n))
    ld = np.zeros(n + 1, np.float64)
    ld[:n] = np.sort(rng.integers(0, max(n // 3, 2), n) / 7.0)
    iprobes = list(range(0, int(li[:n].max(initial=5)) + 6))
    dprobes = [-1.0, 0.0] + [float(x) for x in ld[:n]] + [float(x) + 1e-9 for x in ld[:n]] + [1e9]
    for which, probes, arr in ((0, iprobes, li), (1, iprobes, li), (2, dprobes, ld)):
        for v in probes:
            args = (which, li.ctypes.data, ld.ctypes.data, n, float(v))
            assert lib.grom_cnv_test_bisect(*args) == orc.grom_oracle_bisect(*args), (which, n, v)


def test_oracle_cnv_rows_deterministic_for_a_seed(tmp_path):
    bam, fa = synth(tmp_path, "cnv_small", ["-L", "400000", "-s", "21", "-V", "0.00001", "-W", "15000,60000",
                                             "-Q", "0.05"])
    run_oracle(tmp_path, bam, fa, "a.vcf", ["-V", "1"])
    run_oracle(tmp_path, bam, fa, "b.vcf", ["-V", "1"])
    a = open(tmp_path / "a.vcf").read()
    assert a == open(tmp_path / "b.vcf").read()
    assert a.count("SD:Z:CN:CS") > 0
