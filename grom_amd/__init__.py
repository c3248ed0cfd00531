"""grom_amd -- Python view of the MI355X-native GROM scan library.

The product is the C ABI in ``include/grom_amd.h`` (``grom_amd/lib/libgrom_amd.so``)
and the drop-in CLI ``grom_amd/bin/grom``.  This module only binds them with
ctypes for tests and ``bench.py``; it has no compute of its own and raises if the
HIP library is missing (there is no CPU fallback).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(ROOT)
# GROM_AMD_LIB selects another build of the same library (kernel tuning variants)
LIB_PATH = os.environ.get("GROM_AMD_LIB") or os.path.join(ROOT, "lib", "libgrom_amd.so")
GROM_BIN = os.path.join(ROOT, "bin", "grom")
SYNTH_BIN = os.path.join(ROOT, "bin", "grom_synth")
MAX_TRIALS = 1000
NCOUNT = 40


class Params(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "min_mapq", "rd_min_mapq", "min_base_qual", "min_snv", "ploidy", "gender", "splitread", "rmdup", "vcf",
        "overlap_mult", "sv_list_len", "rmdup_list_len", "read_name_len", "sc_min")] + \
        [(n, C.c_double) for n in ("min_snv_ratio", "min_ave_bq", "snv_rd_min_factor", "high_cov_min_snv_ratio")] + \
        [(n, C.c_int32) for n in ("insert_mean", "insert_min_size", "insert_max_size", "lseq", "one_base_rd_len",
                                  "half_one_base_rd_len", "r14_one_base_rd_len", "r34_one_base_rd_len",
                                  "ranks_stdev", "chr_rd_threshold_factor")] + \
        [(n, C.c_int64) for n in ("min_repeat", "min_blocks", "block_min", "min_rd_window_len", "max_rd_window_len",
                                  "windows_sampling_factor", "dup_threshold_factor")] + \
        [(n, C.c_double) for n in ("min_repeat_stdev", "rd_pval_threshold", "mapq_factor")] + \
        [(n, C.c_int32) for n in ("min_disc", "sc_range", "max_split_loss", "min_sr_len", "max_homopolymer",
                                  "max_ins_range", "sv_list2_len", "pad_sv")] + \
        [(n, C.c_double) for n in ("pval_threshold", "pval_threshold1", "pval_insertion1", "pval_insertion",
                                   "min_sv_ratio", "min_indel_ratio", "max_evidence_ratio", "range_mult",
                                   "max_inv_rd_diff", "min_overlap_ratio")] + \
        [("gen1000_window", C.c_int64)]


class Chrom(C.Structure):
    _fields_ = [("ref", C.c_void_p), ("len", C.c_int64), ("name", C.c_char_p), ("tid", C.c_int32),
                ("n_skip", C.c_int32), ("p_last", C.c_int32), ("cnv", C.c_int32), ("seed", C.c_uint32),
                ("lseq_tail", C.c_int32), ("pad", C.c_int32)]


class Reads(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_cigar_ops", C.c_int64), ("n_bases", C.c_int64)] + \
        [(n, C.c_void_p) for n in ("pos", "flag", "mapq", "mtid", "mpos", "isize", "l_qseq", "cigar_off", "cigar",
                                   "base_off", "seq", "qual", "name_id")] + \
        [("n_aux", C.c_int64), ("aux_idx", C.c_void_p), ("aux", C.c_void_p),
         ("n_drop", C.c_int64), ("drop_pos", C.c_void_p), ("drop_lq", C.c_void_p), ("drop_before", C.c_void_p)]


class Aux(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("pos", "start_adj", "end_adj", "end_adj_indel")] + \
        [("mq", C.c_int16), ("strand", C.c_uint8), ("same_chr", C.c_uint8), ("pad", C.c_int32)]


class SynthSpec(C.Structure):
    """grom_synth_spec: one chromosome of a multi-chromosome synthetic genome."""
    _fields_ = [("n_chr", C.c_int32), ("chrom", C.c_int32), ("chr_len", C.POINTER(C.c_int64)),
                ("names", C.c_char_p), ("coverage", C.c_double), ("read_len", C.c_int32), ("ploidy", C.c_int32),
                ("insert_mean", C.c_double), ("insert_sd", C.c_double), ("dup_frac", C.c_double),
                ("sv_per_mb", C.c_double), ("cnv_rate", C.c_double), ("cnv_min", C.c_int64),
                ("cnv_max", C.c_int64), ("chr_cov", C.POINTER(C.c_double)), ("munmap_frac", C.c_double),
                ("seed", C.c_uint64)]


class Out(C.Structure):
    _fields_ = [("vcf", C.c_void_p), ("vcf_len", C.c_size_t), ("vcf_cap", C.c_size_t),
                ("ctx", C.c_void_p), ("ctx_len", C.c_size_t), ("ctx_cap", C.c_size_t),
                ("side", C.c_void_p), ("side_len", C.c_size_t), ("side_cap", C.c_size_t),
                ("side_written", C.c_int32), ("side_pad", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("ms_total", C.c_double), ("ms_pileup", C.c_double), ("ms_cnv", C.c_double),
                ("cnv_rows", C.c_int64), ("bases_evaluated", C.c_int64),
                ("snv_candidates", C.c_int64), ("mismatch_events", C.c_int64)]


class IndelRec(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("pos", "ins", "ins_len", "del_f", "del_f_len", "del_f_rd", "del_r",
                                         "del_r_len", "del_r_rd", "other_len")] + \
        [("ins_seq", C.c_char * 52), ("pad", C.c_int32)]


class SvRec(C.Structure):
    _fields_ = [("pos", C.c_int32), ("other_len", C.c_int32), ("cnt", C.c_int32 * 10), ("rs", C.c_int32 * 10),
                ("re", C.c_int32 * 10), ("dist", C.c_double * 10), ("ctx_mchr", C.c_int32 * 2)] + \
        [(n, C.c_int32) for n in ("rd_add", "conc", "ins", "mun_f", "mun_r", "pad")]


# numpy view of the breakpoint test-hook records (grom_sv_rec)
SV_DTYPE = np.dtype([("pos", "<i4"), ("other_len", "<i4"), ("cnt", "<i4", 10), ("rs", "<i4", 10), ("re", "<i4", 10),
                     ("dist", "<f8", 10), ("ctx_mchr", "<i4", 2), ("rd_add", "<i4"), ("conc", "<i4"), ("ins", "<i4"),
                     ("mun_f", "<i4"), ("mun_r", "<i4"), ("pad", "<i4")])


# every function declared in include/grom_amd.h, with its ctypes signature
_SIGS = {
    "grom_abi_version": (C.c_int, []),
    "grom_abi_struct_size": (C.c_size_t, [C.c_int]),
    "grom_device_count": (C.c_int, []),
    "grom_last_error": (C.c_char_p, []),
    "grom_set_last_error": (None, [C.c_char_p]),
    "grom_device_mem_free": (C.c_int64, [C.c_int]),
    "grom_dev_init": (C.c_int, [C.c_int, C.POINTER(Params), C.c_void_p, C.c_void_p]),
    "grom_dev_fini": (None, [C.c_int]),
    "grom_ctx_init": (C.c_int, [C.c_int, C.c_int, C.POINTER(Params), C.c_void_p, C.c_void_p]),
    "grom_ctx_set_params": (C.c_int, [C.c_int, C.POINTER(Params)]),
    "grom_scan_chrom": (C.c_int, [C.c_int, C.POINTER(Chrom), C.POINTER(Reads), C.POINTER(Out), C.POINTER(Stats)]),
    "grom_scan_chrom_device": (C.c_int, [C.c_int, C.POINTER(Chrom), C.POINTER(Reads), C.POINTER(Out),
                                         C.POINTER(Stats)]),
    "grom_debug_counts": (C.c_int, [C.c_int, C.POINTER(Chrom), C.POINTER(Reads), C.POINTER(C.c_int32), C.c_void_p,
                                    C.c_int64, C.c_void_p]),
    "grom_debug_indels": (C.c_int64, [C.c_int, C.c_void_p, C.c_int64]),
    "grom_debug_sv": (C.c_int64, [C.c_int, C.c_void_p, C.c_int64]),
    "grom_build_tables": (None, [C.c_int32, C.c_void_p, C.c_void_p]),
    "grom_default_params": (None, [C.POINTER(Params)]),
    "grom_params_set_insert": (None, [C.POINTER(Params), C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "grom_out_free": (None, [C.POINTER(Out)]),
    "grom_fmt_selftest": (C.c_int64, [C.c_int64, C.c_uint64]),
    "grom_bai_build": (C.c_int, [C.c_char_p]),
    "grom_bai_build_device": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int64)]),
    "grom_bai_summary": (C.c_int, [C.c_char_p, C.POINTER(C.c_int64)]),
    "grom_bai_selftest": (C.c_int64, [C.c_char_p, C.c_int64, C.c_uint64, C.POINTER(C.c_int64)]),
    # BGZF block checksums (bgzfcrc_host.cpp, ddecode.hip)
    "grom_bgzf_verify": (C.c_int, [C.c_int]),
    "grom_bgzf_check": (C.c_int, [C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int64]),
    "grom_bgzf_check_device": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int64]),
    "grom_bgzf_crc_twin": (C.c_uint32, [C.c_char_p, C.c_int64, C.c_int64, C.c_uint32]),
    # BGZF written on the device (bgzfwrite.hip; device -1: the host twin, bgzfdef_host.cpp)
    "grom_bgzf_writer_open": (C.c_void_p, [C.c_char_p, C.c_int, C.c_char_p]),
    "grom_bgzf_writer_write": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "grom_bgzf_writer_close": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "grom_bgzf_compress": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int64)]),
    "grom_bgzf_blocks": (C.c_int, [C.c_char_p, C.POINTER(C.c_int64), C.c_int64, C.c_int, C.c_char_p, C.c_int64,
                                   C.POINTER(C.c_int64)]),
    # a VCF sorted, bgzipped and tabix-indexed on the device (vcfsort.hip; device -1: the host twin, vcfsort_host.cpp)
    "grom_vcf_writer_open": (C.c_void_p, [C.c_char_p, C.c_int]),
    "grom_vcf_writer_write": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "grom_vcf_writer_close": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "grom_vcf_tabix": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int64)]),
    "grom_upload": (C.c_int, [C.c_int, C.POINTER(Chrom), C.POINTER(Reads), C.POINTER(Chrom), C.POINTER(Reads)]),
    "grom_synth_batch": (C.c_void_p, [C.c_int64, C.c_double, C.c_int32, C.c_double, C.c_double, C.c_uint64,
                                      C.POINTER(Params)]),
    "grom_synth_chrom": (C.c_void_p, [C.POINTER(SynthSpec), C.POINTER(Params)]),
    "grom_synth_chrom_stream": (C.c_void_p, [C.POINTER(SynthSpec), C.POINTER(Params)]),  # ABI 7
    "grom_reads_digest": (C.c_uint64, [C.POINTER(Reads)]),
    "grom_resident_new": (C.c_void_p, [C.c_int, C.POINTER(Chrom), C.POINTER(Reads), C.POINTER(Chrom),
                                       C.POINTER(Reads)]),
    "grom_resident_bytes": (C.c_int64, [C.c_void_p]),
    "grom_resident_free": (None, [C.c_void_p]),
    "grom_batch_get": (C.c_int, [C.c_void_p, C.POINTER(Chrom), C.POINTER(Reads)]),
    "grom_batch_release": (None, [C.c_void_p]),
    "grom_cli_main": (C.c_int, [C.c_int, C.POINTER(C.c_char_p)]),
    "grom_ctx_postpass": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_char_p), C.c_int32, C.c_int32, C.c_int32,
                                    C.POINTER(Out)]),
    # streamed input (ABI 5)
    "grom_pinned_alloc": (C.c_void_p, [C.c_size_t]),
    "grom_pinned_free": (None, [C.c_void_p]),
    "grom_stage_new": (C.c_void_p, [C.c_int]),
    "grom_stage_free": (None, [C.c_void_p]),
    "grom_stage_begin": (C.c_int, [C.c_void_p, C.c_void_p]),
    "grom_stage_set_ref": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "grom_stage_append": (C.c_int64, [C.c_void_p, C.POINTER(Reads)]),
    "grom_stage_ticket_done": (C.c_int, [C.c_void_p, C.c_int64]),
    "grom_stage_ticket_wait": (C.c_int, [C.c_void_p, C.c_int64]),
    "grom_stage_trim": (C.c_int, [C.c_void_p, C.c_int64]),
    "grom_stage_patch_aux": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(Aux)]),
    "grom_stage_bytes": (C.c_int64, [C.c_void_p]),
    "grom_stage_view": (C.c_int, [C.c_void_p, C.POINTER(Chrom), C.POINTER(Chrom), C.POINTER(Reads)]),
    "grom_scan_chrom_staged": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(Chrom), C.POINTER(Out), C.POINTER(Stats)]),
    "grom_debug_counts_staged": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(Chrom), C.POINTER(C.c_int32), C.c_void_p,
                                           C.c_int64, C.c_void_p]),
    # the reference FASTA on the device, bgzip-compressed or plain (fastadev.hip)
    "grom_fasta_dev_open": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    "grom_fasta_dev_close": (None, [C.c_void_p]),
    "grom_fasta_dev_is_bgzf": (C.c_int, [C.c_void_p]),
    "grom_fasta_dev_kind": (C.c_int, [C.c_void_p]),
    "grom_fasta_allow_gzip": (C.c_int, [C.c_int]),
    "grom_fasta_dev_gzip_stats": (None, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    # the host twin of the device's parallel gzip read (gzip_host.cpp)
    "grom_gzip_inflate_host": (C.c_int, [C.c_char_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "grom_gzip_free": (None, [C.c_void_p]),
    "grom_fasta_dev_index": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "grom_fasta_dev_entry": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int64),
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "grom_fasta_dev_set_index": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_char_p, C.POINTER(C.c_int),
                                           C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "grom_fasta_dev_load": (C.c_int64, [C.c_void_p, C.c_int, C.c_char_p, C.c_int64, C.POINTER(C.c_void_p)]),
    "grom_fasta_dev_release": (None, [C.c_void_p, C.c_void_p]),
    "grom_fasta_dev_times": (None, [C.c_void_p, C.POINTER(C.c_double)]),
    "grom_fasta_host_index": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.c_char_p, C.POINTER(C.c_int),
                                        C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "grom_fasta_host_load": (C.c_int64, [C.c_char_p, C.c_int, C.c_char_p, C.c_int64]),
    "grom_stage_set_ref_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
}

_lib = None


def lib() -> C.CDLL:
    """The loaded HIP library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"grom_amd: {LIB_PATH} missing -- run `make` (or __graft_entry__.build()); "
                               "there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def last_error() -> str:
    return lib().grom_last_error().decode()


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {last_error()}")


BAI_BUILD_COUNTERS = ("records", "blocks", "pieces", "chunks_rewalked", "chunks", "runs", "device_us", "wall_us")


def bai_build(bam: str, bai: str = None, device: int = 0) -> dict:
    """Index `bam` on the GPU `device` into `bai` (default <bam>.bai): the file
    grom_bai_build writes, byte for byte.  Returns the build's counters; raises
    with the library's message (a failed build leaves no file)."""
    out = (C.c_int64 * 8)()
    rc = lib().grom_bai_build_device(os.fsencode(bam), None if bai is None else os.fsencode(bai), device, out)
    check(rc, "grom_bai_build_device")
    return dict(zip(BAI_BUILD_COUNTERS, (int(v) for v in out)))


BGZF_CHECK_COUNTERS = ("blocks", "failing", "first_bad", "inflated_bytes", "pieces", "eof_marker", "device_us", "wall_us")


def verify_bgzf_crc(on: "bool | None") -> "bool | None":
    """Whether every reader of a BGZF file compares each inflated block's
    CRC-32 with the block's trailer (True), does not (False) or follows
    GROM_VERIFY_CRC at each open (None, the default).  Returns the previous
    setting."""
    prev = lib().grom_bgzf_verify(-1 if on is None else int(bool(on)))
    return None if prev < 0 else bool(prev)


def bgzf_check(path: str, device: "int | None" = None, max_bad: int = 4096) -> dict:
    """Every block of the BGZF file `path` (a BAM, a bgzipped FASTA) inflated
    and its CRC-32 compared: on the GPU `device`, or with None on the host
    (one thread, zlib).  Returns the counters of BGZF_CHECK_COUNTERS
    (eof_marker as a bool), `ok`, `bad_off` (up to max_bad failing blocks'
    file offsets, ascending) and `error` (the library's message when a block
    failed, else None).  Raises for a file that is not whole BGZF blocks and
    for device errors."""
    out = (C.c_int64 * 8)()
    bad = (C.c_int64 * max(max_bad, 1))()
    if device is None:
        rc = lib().grom_bgzf_check(os.fsencode(path), out, bad, max_bad)
    else:
        rc = lib().grom_bgzf_check_device(os.fsencode(path), int(device), out, bad, max_bad)
    res = dict(zip(BGZF_CHECK_COUNTERS, (int(v) for v in out)))
    if rc != 0 and res["failing"] == 0:
        check(rc, "grom_bgzf_check" if device is None else "grom_bgzf_check_device")
    res["eof_marker"] = bool(res["eof_marker"])
    res["ok"] = rc == 0
    res["bad_off"] = [int(bad[i]) for i in range(min(res["failing"], max_bad))]
    res["error"] = None if rc == 0 else last_error()
    return res


BGZF_WRITE_COUNTERS = ("blocks", "stored", "fixed", "dynamic", "literal_dynamic", "in_bytes", "out_bytes", "pieces",
                       "device_us", "wall_us")
BGZF_MAX_PAYLOAD = 65280


class BgzfWriter:
    """A BGZF file written through the GPU `device`'s DEFLATE compressor, or
    with None through its host twin (the same bytes).  `gzi`: also bgzip's
    <path>.gzi index.  Use as a context manager; `write(bytes)` may cut the
    stream anywhere.  After the block, `stats` holds BGZF_WRITE_COUNTERS.  An
    exception inside the block still closes the writer."""

    def __init__(self, path: str, device: "int | None" = None, gzi: bool = True):
        self.path, self.stats = path, None
        self._h = lib().grom_bgzf_writer_open(os.fsencode(path), -1 if device is None else int(device),
                                              os.fsencode(path + ".gzi") if gzi else None)
        if not self._h:
            raise RuntimeError(f"grom_bgzf_writer_open failed: {last_error()}")

    def write(self, data: bytes) -> int:
        if self._h is None:
            raise ValueError("write to a closed BgzfWriter")
        data = bytes(data)
        check(lib().grom_bgzf_writer_write(self._h, data, len(data)), "grom_bgzf_writer_write")
        return len(data)

    def close(self) -> dict:
        if self._h is not None:
            out = (C.c_int64 * 10)()
            h, self._h = self._h, None
            rc = lib().grom_bgzf_writer_close(h, out)
            self.stats = dict(zip(BGZF_WRITE_COUNTERS, (int(v) for v in out)))
            check(rc, "grom_bgzf_writer_close")
        return self.stats

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def bgzf_compress(src: str, dst: str, device: "int | None" = None, gzi: bool = True) -> dict:
    """The file `src` as the BGZF file `dst` (and, with gzi, bgzip's
    `dst`.gzi), compressed on the GPU `device` or with None by the host twin,
    which writes the same bytes.  Returns BGZF_WRITE_COUNTERS."""
    if gzi:
        out = (C.c_int64 * 10)()
        rc = lib().grom_bgzf_compress(os.fsencode(src), os.fsencode(dst), -1 if device is None else int(device), out)
        check(rc, "grom_bgzf_compress")
        return dict(zip(BGZF_WRITE_COUNTERS, (int(v) for v in out)))
    with open(src, "rb") as f, BgzfWriter(dst, device, gzi=False) as w:
        while True:
            b = f.read(8 << 20)
            if not b:
                break
            w.write(b)
    return w.stats


VCF_TABIX_COUNTERS = ("rows", "header_lines", "contigs", "inversions", "radix_passes", "bins", "chunks",
                      "linear_windows", "lines_us", "sort_us", "index_us", "wall_us")


class VcfWriter:
    """A VCF written position-sorted, bgzipped and tabix-indexed: `path`,
    `path`.tbi and `path`.gzi, sorted and indexed on the GPU `device`, or with
    None by the host twin (the same bytes).  Use as a context manager;
    `write(bytes)` may cut the stream anywhere.  Everything happens at close;
    after the block, `stats` holds VCF_TABIX_COUNTERS.  A refused stream (no
    final newline, a '#' line after a row, fewer than 8 columns, a POS that is
    not decimal, a row past 2^29) raises with the library's message and leaves
    no file."""

    def __init__(self, path: str, device: "int | None" = 0):
        self.path, self.stats = path, None
        self._h = lib().grom_vcf_writer_open(os.fsencode(path), -1 if device is None else int(device))
        if not self._h:
            raise RuntimeError(f"grom_vcf_writer_open failed: {last_error()}")

    def write(self, data: bytes) -> int:
        if self._h is None:
            raise ValueError("write to a closed VcfWriter")
        data = bytes(data)
        check(lib().grom_vcf_writer_write(self._h, data, len(data)), "grom_vcf_writer_write")
        return len(data)

    def close(self) -> dict:
        if self._h is not None:
            out = (C.c_int64 * 12)()
            h, self._h = self._h, None
            rc = lib().grom_vcf_writer_close(h, out)
            self.stats = dict(zip(VCF_TABIX_COUNTERS, (int(v) for v in out)))
            check(rc, "grom_vcf_writer_close")
        return self.stats

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def vcf_tabix(src: str, dst: str, device: "int | None" = 0) -> dict:
    """The plain VCF `src` as `dst` (BGZF, rows stably sorted by contig in
    order of first appearance, then POS), `dst`.tbi and `dst`.gzi, on the GPU
    `device` or with None by the host twin.  Returns VCF_TABIX_COUNTERS."""
    out = (C.c_int64 * 12)()
    rc = lib().grom_vcf_tabix(os.fsencode(src), os.fsencode(dst), -1 if device is None else int(device), out)
    check(rc, "grom_vcf_tabix")
    return dict(zip(VCF_TABIX_COUNTERS, (int(v) for v in out)))


def bgzf_blocks(payloads, device: "int | None" = None, lead: int = 0) -> list:
    """Test hook: every payload (bytes of at most 65280) as one BGZF block, all
    in one launch on `device` (None: the host twin).  The payloads are laid out
    back to back after `lead` bytes, so their start alignments vary."""
    buf = bytes(lead) + b"".join(payloads)
    offs, o = [lead], lead
    for p in payloads:
        o += len(p)
        offs.append(o)
    n = len(payloads)
    cap = len(buf) + 31 * n + 64
    dst = C.create_string_buffer(cap)
    d_offs = (C.c_int64 * (n + 1))()
    rc = lib().grom_bgzf_blocks(buf, (C.c_int64 * (n + 1))(*offs), n, -1 if device is None else int(device), dst, cap,
                                d_offs)
    check(rc, "grom_bgzf_blocks")
    raw = dst.raw
    return [raw[d_offs[i]:d_offs[i + 1]] for i in range(n)]


FASTA_NAME_LEN = 50
FASTA_HOST_ONLY = -100
FASTA_TIMES = ("read_upload_ms", "inflate_ms", "index_kernels_ms", "load_kernels_ms", "load_d2h_ms", "open_wall_ms",
               "index_wall_ms", "loads_wall_ms")


FASTA_KINDS = ("plain", "bgzf", "gzip")
GZIP_STATS = ("units", "units_guessed", "units_again", "marker_bytes", "members", "max_unit_bytes", "scratch_bytes",
              "groups")
GZIP_TIMES = ("guess_ms", "count_ms", "symbols_ms", "handover_ms", "resolve_ms", "crc_ms")


class FastaHostOnly(RuntimeError):
    """The device loader's "host only" answer (a NUL byte in the text, more
    headers than the host table keeps, or a gzip stream with a stretch too
    long for one lane): the host code has to read the file."""


def allow_gzip_fasta(on: "bool | None") -> "bool | None":
    """Whether a gzip FASTA that is not BGZF is read as it is (True), refused
    (False) or follows GROM_FASTA_GZIP at each open (None, the default).
    Returns the previous setting."""
    prev = lib().grom_fasta_allow_gzip(-1 if on is None else int(bool(on)))
    return None if prev < 0 else bool(prev)


def gzip_inflate_host(data: bytes, chunk_bytes: int = 0, unit_max_bytes: int = 0, guess_mode: int = 1):
    """The host twin of the device's parallel gzip read: (text, stats).  Raises
    FastaHostOnly for a unit over the cap, RuntimeError for a malformed stream."""
    out, n, st = C.c_void_p(), C.c_int64(), (C.c_int64 * 8)()
    rc = lib().grom_gzip_inflate_host(data, len(data), chunk_bytes, unit_max_bytes, guess_mode, C.byref(out), C.byref(n), st)
    stats = dict(zip(GZIP_STATS, (int(v) for v in st)))
    if rc == FASTA_HOST_ONLY:
        raise FastaHostOnly("the gzip read reports: host only")
    check(rc, "grom_gzip_inflate_host")
    try:
        return C.string_at(out, n.value), stats
    finally:
        lib().grom_gzip_free(out)


def _fasta_host_index(path):
    L = lib()
    p = os.fsencode(path)
    n = L.grom_fasta_host_index(p, 0, None, None, None, None, None)
    if n < 0:
        raise RuntimeError(f"grom_fasta_host_index failed ({n}): {last_error()}")
    m = C.c_int64(0)
    names = C.create_string_buffer(FASTA_NAME_LEN * max(n, 1))
    nl, fp, ln = (C.c_int * max(n, 1))(), (C.c_int64 * max(n, 1))(), (C.c_int64 * max(n, 1))()
    L.grom_fasta_host_index(p, n, C.byref(m), names, nl, fp, ln)
    ent = [{"name": names.raw[i * FASTA_NAME_LEN:(i + 1) * FASTA_NAME_LEN].split(b"\0")[0].decode("latin-1"),
            "name_len": nl[i], "file_pos": fp[i], "len": ln[i]} for i in range(n)]
    return {"n": n, "mappable": m.value, "entries": ent}


class FastaDevice:
    """A FASTA (plain, BGZF or -- when allowed -- plain gzip) brought to GPU
    `device` (grom_fasta_dev_*)."""

    def __init__(self, path, device: int = 0):
        self.h = C.c_void_p()
        rc = lib().grom_fasta_dev_open(os.fsencode(path), device, C.byref(self.h))
        if rc == FASTA_HOST_ONLY:
            raise FastaHostOnly("the device open reports: host only")
        check(rc, "grom_fasta_dev_open")

    def close(self):
        if self.h:
            lib().grom_fasta_dev_close(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def bgzf(self) -> bool:
        return bool(lib().grom_fasta_dev_is_bgzf(self.h))

    @property
    def kind(self) -> str:
        """ "plain", "bgzf" or "gzip" """
        return FASTA_KINDS[lib().grom_fasta_dev_kind(self.h)]

    def gzip_stats(self) -> dict:
        """A gzip open's figures (grom_fasta_dev_gzip_stats)."""
        st, ms = (C.c_int64 * 8)(), (C.c_double * 6)()
        lib().grom_fasta_dev_gzip_stats(self.h, st, ms)
        return {**dict(zip(GZIP_STATS, (int(v) for v in st))), **dict(zip(GZIP_TIMES, (float(v) for v in ms)))}

    def entries(self, n):
        out = []
        for i in range(n):
            name = C.create_string_buffer(FASTA_NAME_LEN)
            nl, fp, ln, ll = C.c_int(), C.c_int64(), C.c_int64(), C.c_int64()
            check(lib().grom_fasta_dev_entry(self.h, i, name, C.byref(nl), C.byref(fp), C.byref(ln), C.byref(ll)),
                  "grom_fasta_dev_entry")
            out.append({"name": name.raw.split(b"\0")[0].decode("latin-1"), "name_len": nl.value,
                        "file_pos": fp.value, "len": ln.value, "load_len": ll.value})
        return out

    def index(self) -> dict:
        n, m = C.c_int(), C.c_int64()
        rc = lib().grom_fasta_dev_index(self.h, C.byref(n), C.byref(m))
        if rc == FASTA_HOST_ONLY:
            raise FastaHostOnly("the device index pass reports: host only")
        check(rc, "grom_fasta_dev_index")
        return {"n": n.value, "mappable": m.value, "entries": self.entries(n.value)}

    def set_index(self, table: dict):
        ent = table["entries"]
        n = len(ent)
        names = b"".join(e["name"].encode("latin-1").ljust(FASTA_NAME_LEN, b"\0") for e in ent)
        check(lib().grom_fasta_dev_set_index(self.h, n, table["mappable"], names,
                                             (C.c_int * max(n, 1))(*[e["name_len"] for e in ent]),
                                             (C.c_int64 * max(n, 1))(*[e["file_pos"] for e in ent]),
                                             (C.c_int64 * max(n, 1))(*[e["len"] for e in ent])),
              "grom_fasta_dev_set_index")

    def load_len(self, i: int) -> int:
        r = lib().grom_fasta_dev_load(self.h, i, None, 0, None)
        if r == FASTA_HOST_ONLY:
            raise FastaHostOnly("the device loader reports: host only")
        if r < 0:
            check(int(r), "grom_fasta_dev_load")
        return int(r)

    def load(self, i: int) -> bytes:
        n = self.load_len(i)
        buf = C.create_string_buffer(max(n, 1))
        r = lib().grom_fasta_dev_load(self.h, i, buf, n, None)
        if r == FASTA_HOST_ONLY:
            raise FastaHostOnly("the device loader reports: host only")
        if r < 0:
            check(int(r), "grom_fasta_dev_load")
        return buf.raw[:n]

    def times(self) -> dict:
        ms = (C.c_double * 8)()
        lib().grom_fasta_dev_times(self.h, ms)
        return dict(zip(FASTA_TIMES, (float(v) for v in ms)))


def fasta_index(path, device: "int | None" = None) -> dict:
    """The FASTA index (find_genome_length): {"n", "mappable", "entries": [{"name",
    "name_len", "file_pos", "len"(, "load_len")}]}.  device=None runs the host
    code (a BGZF file inflated on the host); else the device pass, which raises
    FastaHostOnly where only the host code can read the file."""
    if device is None:
        return _fasta_host_index(path)
    with FastaDevice(path, device) as f:
        return f.index()


def fasta_load(path, i: int, device: "int | None" = None, host_fallback: bool = True) -> bytes:
    """Entry i's bytes as the loader keeps them.  device=None runs the host
    code.  On a device, "host only" takes the host path as the CLI does
    (host_fallback=False: raises FastaHostOnly)."""
    if device is not None:
        try:
            with FastaDevice(path, device) as f:
                f.index()
                return f.load(i)
        except FastaHostOnly:
            if not host_fallback:
                raise
    L = lib()
    p = os.fsencode(path)
    n = L.grom_fasta_host_load(p, i, None, 0)
    if n < 0:
        raise RuntimeError(f"grom_fasta_host_load failed ({n}): {last_error()}")
    buf = C.create_string_buffer(max(n, 1))
    L.grom_fasta_host_load(p, i, buf, n)
    return buf.raw[:n]


def default_params() -> Params:
    p = Params()
    lib().grom_default_params(C.byref(p))
    return p


def build_tables(min_mapq: int = 20):
    """(hez, mq) binomial tables exactly as a `-q min_mapq` run uses them."""
    hez = np.zeros((MAX_TRIALS + 1, MAX_TRIALS + 1), np.float64)
    mq = np.zeros_like(hez)
    lib().grom_build_tables(min_mapq, hez.ctypes.data, mq.ctypes.data)
    return hez, mq


class Device:
    """One initialised GPU (grom_dev_init / grom_dev_fini)."""

    def __init__(self, device: int, params: Params, slot: "int | None" = None):
        """slot: the library context to use (default: the device number); a
        second slot on the same device scans concurrently with the first."""
        self.device = device if slot is None else slot  # the slot every call names
        self.gpu = device
        self.params = params
        self.hez, self.mq = build_tables(params.min_mapq)
        check(lib().grom_ctx_init(self.device, device, C.byref(params), self.hez.ctypes.data, self.mq.ctypes.data),
              "grom_ctx_init")

    def close(self):
        lib().grom_dev_fini(self.device)

    def scan(self, chrom: Chrom, reads: Reads, device_resident: bool = False, out: "Out | None" = None):
        """Scan one chromosome; returns (VCF text, Stats).  With a caller-owned
        `out` (reused across calls, freed with grom_out_free) the text stays
        in out.vcf and the first element is its length instead."""
        own = out is None
        if own:
            out = Out()
        else:
            out.vcf_len = 0
            out.ctx_len = 0
        st = Stats()
        fn = lib().grom_scan_chrom_device if device_resident else lib().grom_scan_chrom
        check(fn(self.device, C.byref(chrom), C.byref(reads), C.byref(out), C.byref(st)), "scan")
        if not own:
            return out.vcf_len, st
        text = C.string_at(out.vcf, out.vcf_len).decode() if out.vcf_len else ""
        lib().grom_out_free(C.byref(out))
        return text, st

    def scan_rows(self, chrom: Chrom, reads: Reads, device_resident: bool = False):
        """Scan one chromosome; returns (VCF text, raw CTX rows, Stats).  The raw
        CTX rows of every chromosome feed ctx_postpass."""
        out, st = Out(), Stats()
        fn = lib().grom_scan_chrom_device if device_resident else lib().grom_scan_chrom
        check(fn(self.device, C.byref(chrom), C.byref(reads), C.byref(out), C.byref(st)), "scan")
        vcf = C.string_at(out.vcf, out.vcf_len).decode() if out.vcf_len else ""
        ctx = C.string_at(out.ctx, out.ctx_len).decode() if out.ctx_len else ""
        lib().grom_out_free(C.byref(out))
        return vcf, ctx, st

    def upload(self, chrom: Chrom, reads: Reads):
        dc, dr = Chrom(), Reads()
        check(lib().grom_upload(self.device, C.byref(chrom), C.byref(reads), C.byref(dc), C.byref(dr)), "upload")
        return dc, dr

    def debug_counts(self, chrom: Chrom, reads: Reads):
        lo = max(self.params.one_base_rd_len // 4 + 1, 2 * self.params.insert_max_size + 1)
        n_eval = max(chrom.p_last - lo + 1, 0)
        cnt = np.zeros((max(n_eval, 1), NCOUNT), np.int32)
        caf = np.zeros((3, chrom.len), np.int32)
        first = C.c_int32(0)
        check(lib().grom_debug_counts(self.device, C.byref(chrom), C.byref(reads), C.byref(first), cnt.ctypes.data,
                                      cnt.size, caf.ctypes.data), "grom_debug_counts")
        return cnt[:n_eval], caf


class Resident:
    """A chromosome's inputs kept in HBM (grom_resident_new); scan them from any
    context on the same device with Device.scan(..., device_resident=True)."""

    def __init__(self, device: int, chrom: Chrom, reads: Reads):
        self.chrom, self.reads = Chrom(), Reads()
        self.h = lib().grom_resident_new(device, C.byref(chrom), C.byref(reads), C.byref(self.chrom),
                                         C.byref(self.reads))
        if not self.h:
            raise RuntimeError(f"grom_resident_new failed: {last_error()}")
        self.bytes = lib().grom_resident_bytes(self.h)
        # the name is host text owned by the source batch: keep a copy here
        self.chrom.name = bytes(chrom.name or b"")

    def close(self):
        if self.h:
            lib().grom_resident_free(self.h)
            self.h = None


class SynthBatch:
    """A synthetic chromosome and the read batch its scan ingests (host memory)."""

    def __init__(self, length: int, coverage: float = 30.0, read_len: int = 150, insert_mean: float = 500.0,
                 insert_sd: float = 50.0, seed: int = 2, params: Params | None = None, _handle=None):
        self.params = params if params is not None else default_params()
        self.h = _handle if _handle is not None else lib().grom_synth_batch(
            length, coverage, read_len, insert_mean, insert_sd, seed, C.byref(self.params))
        if not self.h:
            raise RuntimeError("grom_synth_batch failed")
        self.chrom, self.reads = Chrom(), Reads()
        check(lib().grom_batch_get(self.h, C.byref(self.chrom), C.byref(self.reads)), "grom_batch_get")

    @classmethod
    def genome_chrom(cls, lengths, chrom: int, params: Params, names=None, coverage: float = 30.0,
                     read_len: int = 150, ploidy: int = 2, insert_mean: float = 500.0, insert_sd: float = 50.0,
                     dup_frac: float = 0.0, sv_per_mb: float = 0.0, cnv_rate: float = 0.0,
                     cnv_range=(0, 0), chr_cov=None, munmap_frac: float = 0.002, seed: int = 2,
                     stream: bool = False) -> "SynthBatch":
        """Chromosome `chrom` of a multi-chromosome synthetic genome (grom_synth_chrom).
        `params` keeps genome-wide insert statistics once set (see include/grom_amd.h).
        stream=True: as the chromosome's scan sees it inside the genome's BAM
        (grom_synth_chrom_stream: the serial stream's Q1 drops and pending-record length)."""
        arr = (C.c_int64 * len(lengths))(*lengths)
        cov = (C.c_double * len(lengths))(*chr_cov) if chr_cov is not None else None
        sp = SynthSpec(len(lengths), chrom, arr, ",".join(names).encode() if names else None, coverage, read_len,
                       ploidy, insert_mean, insert_sd, dup_frac, sv_per_mb, cnv_rate, cnv_range[0], cnv_range[1],
                       cov, munmap_frac, seed)
        fn = lib().grom_synth_chrom_stream if stream else lib().grom_synth_chrom
        h = fn(C.byref(sp), C.byref(params))
        if not h:
            raise RuntimeError(f"grom_synth_chrom failed for chromosome {chrom}: {last_error()}")
        return cls(lengths[chrom], params=params, _handle=h)

    def close(self):
        if self.h:
            lib().grom_batch_release(self.h)
            self.h = None

    @property
    def n_reads(self) -> int:
        return self.reads.n

    @property
    def n_bases(self) -> int:
        return self.reads.n_bases


def ctx_postpass(raw: str, target_names, insert_max: int, lseq: int) -> str:
    """main's translocation post-pass (grom_ctx_postpass) over the raw CTX rows
    of every chromosome in chromosome order: the BND rows of .ctx.vcf."""
    names = (C.c_char_p * max(len(target_names), 1))(*[n.encode() for n in target_names])
    out = Out()
    data = raw.encode()
    check(lib().grom_ctx_postpass(data, len(data), names, len(target_names), insert_max, lseq, C.byref(out)),
          "grom_ctx_postpass")
    text = C.string_at(out.ctx, out.ctx_len).decode() if out.ctx_len else ""
    lib().grom_out_free(C.byref(out))
    return text


def cli_main(args, env=None, cwd=None) -> int:
    """Run the drop-in CLI in this process (loads the HIP library here)."""
    saved_env, saved_cwd = dict(os.environ), os.getcwd()
    try:
        if env:
            os.environ.update(env)
        if cwd:
            os.chdir(cwd)
        argv = [b"grom"] + [str(a).encode() for a in args]
        arr = (C.c_char_p * (len(argv) + 1))(*argv, None)
        return lib().grom_cli_main(len(argv), arr)
    finally:
        os.chdir(saved_cwd)
        os.environ.clear()
        os.environ.update(saved_env)


def run_grom(args, env=None, check_rc=True, timeout=600):
    """Run the drop-in CLI as a subprocess (GPU)."""
    e = dict(os.environ)
    if env:
        e.update(env)
    r = subprocess.run([GROM_BIN] + list(args), env=e, capture_output=True, text=True, timeout=timeout)
    if check_rc and r.returncode != 0:
        raise RuntimeError(f"grom failed ({r.returncode}): {r.stdout[-2000:]} {r.stderr[-2000:]}")
    return r


def run_synth(prefix, *args, timeout=600):
    r = subprocess.run([SYNTH_BIN, "-o", prefix] + [str(a) for a in args], capture_output=True, text=True,
                       timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError(f"grom_synth failed: {r.stderr}")
    return prefix + ".bam", prefix + ".fa"
