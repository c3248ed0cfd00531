// cnvcall.h -- the host arithmetic of the read-depth CNV path (cnvcall.cpp) and
// the plain structs it shares with the kernels (cnv.hip).  No HIP here: every
// function takes and returns values, so the sanitizer builds replay it on
// recorded inputs without a device (GROM_CNV_HOST_DUMP, san_driver cnvhost).
// cnv.hip launches, copies and calls into these, as sv.hip does with svcall.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/grom_amd.h"

namespace cnvcall {

// ---- fixed parameters of the reference (not on its command line) ----
constexpr int NBINS = 101;                 // g_num_gc_bins, GROM.c:947
constexpr int REP_SEGS = 10;               // g_repeat_segments, GROM.c:732
// g_sample_lists_len, GROM.c:725; GROM_SAMPLE_LISTS_LEN lowers it (test hook:
// the reservoir draws of GROM.c:18292/18393 then fire on small inputs, and
// the oracle reads the same variable)
inline long sample_len() {
    const char *e = getenv("GROM_SAMPLE_LISTS_LEN");
    const long x = e ? atol(e) : 0;
    return (x > 0 && x < 100000) ? x : 100000L;
}
constexpr long REDUCTION = 1;              // g_genome_reduction_factor, GROM.c:726
constexpr long BLOCK_FACTOR = 4;           // g_block_factor, GROM.c:738
constexpr long BLOCK_UNIT = 10000;         // g_block_unit_size, GROM.c:740
constexpr int MIN_ACGT = 99;               // g_insert_min_acgt, GROM.c:926
constexpr long NO_COMBINE = 100;           // g_rd_no_combine_min_windows, GROM.c:929
constexpr long RD_MIN_WINDOWS = 20;        // g_rd_min_windows, GROM.c:928
constexpr double PLOIDY_NUM = 0.6;         // g_ploidy_threshold_numerator, GROM.c:939
constexpr double STDEV_STEP = 0.01;        // g_stdev_step, GROM.c:940
constexpr int MAX_BLOCK_LIST = 10000;      // max_block_list_len, GROM.c:633
constexpr int HIST_MAX = 4096;             // exact depth histogram for the chromosome variance

// flag byte per position
constexpr uint8_t F_LOW = 1;    // ddd_rd_low_acgt_or_windows_list != 0
constexpr uint8_t F_GUARD = 2;  // z-scored / windowed base (GROM.c:18765 condition)

struct Tables {  // device copy of the per-chromosome bin statistics
    int32_t off[2][NBINS], cnt[2][NBINS];
    int64_t wins[2][NBINS];
    double ave[2][NBINS], sdv[2][NBINS], thr[2][2][NBINS];  // thr[0]=del, thr[1]=dup
    double p2s_p[1001], p2s_sd[1001];
    int32_t n_p2s;
};
constexpr size_t TABLES_BYTES = offsetof(Tables, n_p2s) + sizeof(int32_t);  // without the tail padding

struct RepeatRec {
    int64_t start, end, rd;  // [start, end), depth sum over it
    int32_t type, pad;
};

struct GatherRange {
    int64_t start, count, stride, out;
};

struct WinPiece {
    int64_t start, count;
};
struct WinDesc {
    int64_t p0, n0, p1, n1, p2, n2;  // the first three pieces inline (the common case)
    int64_t piece0, n_pieces, ntot;  // all pieces: [piece0, piece0 + n_pieces) of the piece list, ntot bases
    int64_t row;
};

struct CallRec {
    int64_t p, ce;
    double stdevs;
    int32_t m, pad;
};

// glibc random()/rand() (TYPE_3, stdlib/random_r.c) for grom_rand, GROM.c:1185
struct GlibcRand {
    int32_t st[31];
    int f = 3, r = 0;
    explicit GlibcRand(uint32_t seed) {
        if (seed == 0) seed = 1;
        st[0] = (int32_t)seed;
        int32_t word = (int32_t)seed;  // int32_t in glibc's __srandom_r
        for (int i = 1; i < 31; i++) {
            long hi = word / 127773, lo = word % 127773;
            word = (int32_t)(16807 * lo - 2836 * hi);
            if (word < 0) word += 2147483647;
            st[i] = word;
        }
        for (int i = 0; i < 310; i++) next();
    }
    int next() {
        uint32_t v = (uint32_t)st[f] + (uint32_t)st[r];
        st[f] = (int32_t)v;
        if (++f >= 31) { f = 0; ++r; } else if (++r >= 31) r = 0;
        return (int)(v >> 1);
    }
    long grom_rand(long mx) {  // GROM.c:1185-1201
        long v = 0, c = 1, t;
        while (c < mx) {
            t = (next() % 10) * c;
            while (t + v >= mx) t = (next() % 10) * c;
            v += t;
            c *= 10;
        }
        return v;
    }
};

// qsort(double[], cmpfunc) of glibc 2.12 (msort.c) with the reference's int
// comparator reading each double's low 32 bits; msort_lo_par sorts
// the halves of the top `depth` levels on their own threads, same merges
int dcmp_lo(double a, double b);
void msort_lo(double *b, size_t n, double *t);
void msort_lo_par(double *b, size_t n, double *t, int depth);
// sort of small non-negative ints (read depths): counting sort, same result
// as the reference's qsort with cmpfunc on these values
void sort_depths(std::vector<int> &v);

// host views of the per-position values of gathered ranges (k_cnv_gather)
struct GatherView {
    const uint8_t *gc = nullptr, *ac = nullptr, *flag = nullptr;
    const int32_t *mq = nullptr, *rd = nullptr, *low = nullptr, *rt = nullptr;
};

// ---- depth statistics, GROM.c:16645-16775 ----
struct DepthStats {
    double chr_ave = 0;  // chromosome depth mean over ACGT-rich bases
    long chr_cnt = 0;
    double rave[10] = {0}, rsd[10] = {0};  // per repeat type: capped depth mean and stdev
    long rcnt[10] = {0};
};
// hacc: block depth sum and count, chromosome depth sum and count (k_cnv_blocks)
DepthStats depth_stats(const unsigned long long hacc[4], const std::vector<RepeatRec> &reps);
// the most biased repeat type given the chromosome depth stdev, or -1
int biased_repeat(const DepthStats &D, const grom_params &P, double sd);
// the same decided from the exact depth histogram's bound on that stdev
// (hist[HIST_MAX]: deeper bases); false when the bound cannot decide
bool biased_repeat_from_hist(const DepthStats &D, const grom_params &P, const std::vector<unsigned int> &hist,
                             int *biased);
// the chromosome depth stdev as the reference sums it, in base order over [lo, hi)
double depth_sd_serial(const DepthStats &D, const int32_t *rd, const int32_t *low, const uint8_t *acw, int64_t n);

// ---- low-variance sample blocks, GROM.c:16784-16993: blk_total holds
// len / BLOCK_UNIT block depth totals; out g_lowvar_block_sample_*_list ----
void lowvar_blocks(const grom_params &P, const unsigned long long hacc[4], const std::vector<int64_t> &blk_total,
                   int64_t len, std::vector<long> &ss, std::vector<long> &se);

// ---- sampling, GROM.c:18284-18641 ----
// every insert_mean/2-th base of the sample blocks; the biased type's repeats
// with insert_mean/2 bases on either side
std::vector<GatherRange> bin_sample_ranges(const std::vector<long> &ss, const std::vector<long> &se, long half,
                                           int64_t *total);
std::vector<GatherRange> repeat_ranges(const std::vector<RepeatRec> &reps, int biased, long half, int64_t *total);

// a capped sample list with the reference's reservoir replacement past the cap
struct Reservoir {
    GlibcRand rng;
    long cap;
    long over = 0, repl = 0;  // draws past a full list, replacements (GROM_CNV_STATS)
    Reservoir(uint32_t seed, long cap_) : rng(seed), cap(cap_) {}
    void push(std::vector<int> &list, long &idx, long &all, int v) {
        if (idx < cap) {
            list.push_back(v);
            idx += 1;
            all += 1;
        } else {
            over++;
            if (rng.grom_rand(all) == 0) { list[rng.grom_rand(idx)] = v; repl++; }
            all += 1;
        }
    }
};
struct BinSamples {  // [high/low MAPQ class][GC bin]
    std::vector<std::vector<int>> smp[2] = {std::vector<std::vector<int>>(NBINS), std::vector<std::vector<int>>(NBINS)};
    long idx[2][NBINS] = {{0}}, all[2][NBINS] = {{0}};
};
struct RepeatSamples {  // by segment of the repeat's flank (REP_SEGS - 1: inside)
    std::vector<std::vector<int>> smp = std::vector<std::vector<int>>(REP_SEGS);
    long idx[REP_SEGS] = {0}, all[REP_SEGS] = {0};
    double ave[REP_SEGS] = {0}, sd[REP_SEGS] = {0};
};
// (the most-biased-repeat samples come first in the reference and draw from
// the same generator, GROM.c:18284-18330)
void sample_repeats(Reservoir &R, const std::vector<GatherRange> &rrg, long half, const GatherView &g,
                    RepeatSamples &out);
void sample_bins(Reservoir &R, int64_t total, const GatherView &g, int rd_min_mapq, BinSamples &out);
void borrow_thin_bins(BinSamples &B, long sample_cap);  // GROM.c:18480-18548
void repeat_segment_stats(RepeatSamples &R);             // GROM.c:18336-18367
// bin statistics, GROM.c:18560-18641 -> Tables and the flat sample array
void bin_stats(const BinSamples &B, const grom_params &P, Tables &T, std::vector<int32_t> &flat);

// ---- p values.  Two functions on purpose: the table's t is 1/(1 + pp*x)
// (find_disc_svs, GROM.c:20705-20748) and the row's is the reference's own
// 1/(1 + pp + x) (GROM.c:17139-17300).  Both are kept as the reference has them. ----
void pval2sd_table(Tables &T);
double row_pvalue(double stdevs);

// ---- window means by length, GROM.c:18967-19018: the sampled windows ----
struct WindowPlan {
    std::vector<WinDesc> wds;
    std::vector<WinPiece> wps;
    std::vector<int64_t> rlen;
};
WindowPlan window_plan(const std::vector<long> &ss, const std::vector<long> &se, const grom_params &P);
// wsd per window length (GROM.c:19162) and its minima over the next 64 and 512
// lengths (L + 2 entries each, the last 0)
std::vector<double> window_sd(const std::vector<double> &wtot, const std::vector<int64_t> &wcnt, int64_t ML, int64_t L);
void window_sd_minima(const std::vector<double> &wsd, int64_t L, std::vector<double> &wmin,
                      std::vector<double> &wmin512);

// ---- most-biased repeat z override, GROM.c:19022-19150: positions ascending,
// each once, the reference's last write to a base kept ----
void repeat_z_override(const std::vector<GatherRange> &rrg, long half, const GatherView &g, const RepeatSamples &R,
                       const Tables &T, const grom_params &P, double dup_factor, std::vector<int64_t> &pos,
                       std::vector<double> &z);

// ---- rows, GROM.c:17139-17300, 20024-20228 ----
struct KeptCall {
    size_t idx;  // into the kind's valid calls
    double pv;
};
std::vector<KeptCall> keep_calls(const std::vector<CallRec> &calls, double pval_threshold);
std::vector<GatherRange> call_ranges(const std::vector<CallRec> &calls, const std::vector<KeptCall> &keep,
                                     int64_t *total);
// copy number and its spread for every range of per-base ratios (HUGE_VAL: no
// ratio at that base); independent per call, shared among host threads
unsigned copy_numbers(const double *ratios, const std::vector<GatherRange> &rg, int ploidy, std::vector<double> &cn,
                      std::vector<double> &cs);
// one kind's rows (kind 0 DEL, 1 DUP), -f with its column header or VCF
int64_t format_rows(std::string &rows, const grom_params &P, int kind, const char *chr_name,
                    const std::vector<CallRec> &calls, const std::vector<KeptCall> &keep,
                    const std::vector<double> &cn, const std::vector<double> &cs);

// ---- test hook GROM_CNV_HOST_DUMP=<dir>: one chromosome's inputs to and
// outputs of the functions above as tagged blobs (tools/record_cnv_host.sh),
// replayed by grom_cnv_host_replay ----
struct HostDump {
    FILE *f = nullptr;
    HostDump(const char *chr_name);  // opens <dir>/<chr>.cnvh when the variable is set
    ~HostDump();
    explicit operator bool() const { return f != nullptr; }
    void put(const char *tag, const void *p, size_t bytes);
    template <class T>
    void vec(const char *tag, const std::vector<T> &v) { put(tag, v.data(), sizeof(T) * v.size()); }
};

}  // namespace cnvcall

extern "C" {
// replays one record through the functions above; the number of recorded
// outputs that differ (0: all equal), negative: unreadable record
int64_t grom_cnv_host_replay(const char *path);
// test hooks (tests/test_oracle_cnv.py)
void grom_cnv_test_rand(uint32_t seed, int n, int32_t *out);
void grom_cnv_test_msort_lo(double *v, int64_t n);
long grom_cnv_test_bisect(int which, const int *l, const double *ld, long n, double v);
}
