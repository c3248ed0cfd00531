// vcfsort_host.h -- the host half of the sorting, indexing VCF writer
// (vcfsort_host.cpp, no HIP): the whole host twin, and the
// steps that run on the host on either path -- the contig names, the refusals'
// messages, the .tbi from the device's runs.  vcfsort.hip and the sanitizer
// program (tools/tbi_check.cpp) call them.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

// one run of sorted rows with one contig and bin: its first row's virtual
// offset and its last row's end
struct VsRun {
    int32_t cid;
    uint32_t bin;
    uint64_t beg, end;
};
// a contig's rows in the sorted file
struct VsSpan {
    uint64_t beg, end, rows;
};
// out[12] of grom_vcf_writer_close
enum { VS_O_ROWS, VS_O_HEADER, VS_O_CONTIGS, VS_O_INVERSIONS, VS_O_PASSES, VS_O_BINS, VS_O_CHUNKS, VS_O_WINDOWS,
       VS_O_US_LINES, VS_O_US_SORT, VS_O_US_INDEX, VS_O_US_WALL };

// the message of a refused line (kind: vcfsort.h's VS_E_*; line counts from 1)
void vs_refusal(int kind, int64_t line, char *err, size_t cap);
extern const char *const VS_MSG_NO_NEWLINE;

// the first refused line of text[0, n), as the writer words it: 1 with err set, 0 when nothing is refused
int vs_first_refusal(const uint8_t *text, int64_t n, char *err, size_t cap);

// The runs of rows with one CHROM (head[r] = the offset of the run's first
// row in the stream, which lies in chunks of `chunk` bytes) to contig ids in
// order of first appearance: run_cid[r], the NUL-terminated names back to
// back.  Returns the number of contigs.
int32_t vs_map_names(const uint8_t *const *chunks, int64_t chunk, const int64_t *head, int64_t n_runs,
                     std::vector<uint32_t> &run_cid, std::string &names);

// the digits (8 bits each, 0..7) in which the keys differ, given the OR of key ^ key[0]
int vs_passes(uint64_t diff, int digit[8]);

// `data` as a BGZF file at `path` (payloads of 65280 bytes through the
// compressor's host twin, the EOF marker); coff (may be NULL) takes every
// block's file offset and the marker's, gzi_path (may be NULL) bgzip's index.
int vs_bgzf_file(const char *path, const uint8_t *data, int64_t n, const char *gzi_path, std::vector<int64_t> *coff);

// The .tbi at `path`: the runs in file order through the BAI accumulator
// (merge rule, pseudo-bin, window filling), lin[lin_base[c] .. lin_base[c + 1])
// the contig's windows (VS_NONE: no row), BGZF-compressed by the host twin.
// counts[3] = {bins, chunks, windows}.  0 or -1 with err set.
int vs_write_tbi(const char *path, const std::string &names, int32_t n_ref, const VsRun *runs, int64_t n_runs,
                 const uint64_t *lin, const int64_t *lin_base, const VsSpan *span, int64_t counts[3], char *err,
                 size_t cap);

// the three temporary files renamed to path, path.tbi and path.gzi (or, with !ok, removed)
int vs_commit(const std::string &path, const std::string &tmp_gz, const std::string &tmp_tbi, const std::string &tmp_gzi,
              bool ok, char *err, size_t cap);

// The host twin: text[0, n) sorted and indexed into path, path.tbi, path.gzi.
// 0 or a GROM_E_* code with err set; a failure leaves no file.
int vs_host_run(const uint8_t *text, int64_t n, const char *path, int64_t out[12], char *err, size_t cap);
