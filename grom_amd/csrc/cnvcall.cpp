// cnvcall.cpp -- the host arithmetic of the read-depth CNV path (cnvcall.h):
// depth statistics and the biased-repeat decision, the sample blocks, the
// GC-bin and repeat-segment samplers, bin statistics, the pval2sd table, the
// window plan, the repeat z override, wsd and its minima, copy numbers and
// rows.  Every double is produced in the reference's operation order
// (compiled with -ffp-contract=off).  No HIP calls.
#include "cnvcall.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <thread>

#include "cnv_bisect.h"

namespace cnvcall {

int dcmp_lo(double a, double b) {
    uint32_t x, y;
    memcpy(&x, &a, 4);
    memcpy(&y, &b, 4);
    return (int32_t)(x - y);
}
void msort_lo(double *b, size_t n, double *t) {
    if (n <= 1) return;
    size_t n1 = n / 2, n2 = n - n1;
    double *b1 = b, *b2 = b + n1;
    msort_lo(b1, n1, t);
    msort_lo(b2, n2, t);
    double *o = t;
    while (n1 > 0 && n2 > 0) {
        if (dcmp_lo(*b1, *b2) <= 0) { *o++ = *b1++; --n1; }
        else { *o++ = *b2++; --n2; }
    }
    if (n1 > 0) memcpy(o, b1, n1 * sizeof(double));
    memcpy(b, t, (n - n2) * sizeof(double));
}

// the same merge sort with the two halves of the top `depth` levels sorted on
// their own threads (each with its own half of the scratch): the same
// operations on the same data, so the same order -- which matters, since the
// reference's comparator (low 32 bits, wrapping difference) is not a total
// order and only this exact merge sequence reproduces its result
void msort_lo_par(double *b, size_t n, double *t, int depth) {
    if (depth <= 0 || n < (1u << 16)) {
        msort_lo(b, n, t);
        return;
    }
    size_t n1 = n / 2, n2 = n - n1;
    double *b1 = b, *b2 = b + n1;
    std::thread th([=] { msort_lo_par(b1, n1, t, depth - 1); });
    msort_lo_par(b2, n2, t + n1, depth - 1);
    th.join();
    double *o = t;
    while (n1 > 0 && n2 > 0) {
        if (dcmp_lo(*b1, *b2) <= 0) { *o++ = *b1++; --n1; }
        else { *o++ = *b2++; --n2; }
    }
    if (n1 > 0) memcpy(o, b1, n1 * sizeof(double));
    memcpy(b, t, (n - n2) * sizeof(double));
}

void sort_depths(std::vector<int> &v) {
    if (v.size() < 2) return;
    int mx = 0;
    for (int x : v) {
        if (x < 0) { std::sort(v.begin(), v.end()); return; }
        mx = std::max(mx, x);
    }
    if (mx > (1 << 20)) { std::sort(v.begin(), v.end()); return; }
    std::vector<uint32_t> h((size_t)mx + 1, 0);
    for (int x : v) h[x]++;
    size_t k = 0;
    for (int x = 0; x <= mx; x++)
        for (uint32_t c = 0; c < h[x]; c++) v[k++] = x;
}

// ---------------- depth statistics ----------------

DepthStats depth_stats(const unsigned long long hacc[4], const std::vector<RepeatRec> &reps) {
    DepthStats D;
    // chromosome depth mean over ACGT-rich bases, GROM.c:16645-16660: a double
    // sum of integers below 2^53, so the exact integer total is the same value
    D.chr_cnt = (long)hacc[3];
    if (D.chr_cnt > 0) D.chr_ave = (double)hacc[2] / D.chr_cnt;
    const double chr_ave = D.chr_ave;
    // repeat-type depth, GROM.c:16686-16775
    std::vector<double> rrl(reps.size());
    for (size_t i = 0; i < reps.size(); i++) {
        rrl[i] = (double)reps[i].rd / (reps[i].end - reps[i].start);
        D.rave[reps[i].type] += (rrl[i] < 2 * chr_ave) ? rrl[i] : 2 * chr_ave;
        D.rcnt[reps[i].type] += 1;
    }
    for (int t = 0; t < 10; t++) D.rave[t] = D.rave[t] / (double)D.rcnt[t];
    for (size_t i = 0; i < reps.size(); i++) {
        int t = reps[i].type;
        double v = (rrl[i] < 2 * chr_ave) ? rrl[i] : 2 * chr_ave;
        D.rsd[t] += (v - D.rave[t]) * (v - D.rave[t]);
    }
    for (int t = 0; t < 10; t++) D.rsd[t] = D.rcnt[t] > 1 ? sqrt(D.rsd[t] / ((double)D.rcnt[t] - 1.0)) : 0;
    return D;
}

int biased_repeat(const DepthStats &D, const grom_params &P, double sd) {
    int b = -1;
    long bc = 0;
    for (int t = 0; t < 10; t++)
        if (D.rcnt[t] > NO_COMBINE && (D.rave[t] + (P.min_repeat_stdev * D.rsd[t])) < D.chr_ave &&
            (D.chr_ave - (P.min_repeat_stdev * sd)) > D.rave[t] && D.rcnt[t] > bc) {
            b = t;
            bc = D.rcnt[t];
        }
    return b;
}

// The chromosome depth stdev (GROM.c:16664-16685) is a sequential double
// sum in base order, and it only feeds the comparison in biased_repeat.  The
// terms are the reference's own doubles; only their summation order differs,
// so the reference's sum lies within gamma(n) = n*u/(1-n*u) (relative) of the
// exact sum of the histogram's terms.  When every comparison comes out the
// same at both ends of that interval it is decided; otherwise (or when the
// depth histogram cannot hold twice the mean) the caller redoes the sum in
// base order (depth_sd_serial).
bool biased_repeat_from_hist(const DepthStats &D, const grom_params &P, const std::vector<unsigned int> &hist,
                             int *biased) {
    const double chr_ave = D.chr_ave;
    const long chr_cnt = D.chr_cnt;
    if (chr_cnt <= 1) {
        *biased = biased_repeat(D, P, 0.0);
        return true;
    }
    if (2 * chr_ave >= HIST_MAX) return false;
    long double s = 0;
    for (int v = 0; v < HIST_MAX; v++) {
        if (!hist[v]) continue;
        double term = (v < 2 * chr_ave) ? (v - chr_ave) * (v - chr_ave) : chr_ave * chr_ave;
        s += (long double)term * hist[v];
    }
    s += (long double)hist[HIST_MAX] * (long double)(chr_ave * chr_ave);
    const long double nu = (long double)chr_cnt * 0x1p-53L;
    const long double g = nu / (1.0L - nu) + 1e-15L;  // + histogram rounding and sqrt/div ulps
    const double sd_lo = (double)sqrtl(s * (1.0L - g) / ((long double)chr_cnt - 1.0L));
    const double sd_hi = (double)sqrtl(s * (1.0L + g) / ((long double)chr_cnt - 1.0L));
    const int b_lo = biased_repeat(D, P, nextafter(sd_lo, 0.0)), b_hi = biased_repeat(D, P, nextafter(sd_hi, INFINITY));
    if (b_lo != b_hi) return false;
    *biased = b_lo;
    return true;
}

double depth_sd_serial(const DepthStats &D, const int32_t *rd, const int32_t *low, const uint8_t *acw, int64_t n) {
    const double chr_ave = D.chr_ave;
    double sd = 0;
    for (int64_t i = 0; i < n; i++) {
        if (acw[i] < MIN_ACGT) continue;
        const int r = rd[i] + low[i];
        if (r < 2 * chr_ave) sd += (r - chr_ave) * (r - chr_ave);
        else sd += chr_ave * chr_ave;
    }
    return sqrt(sd / ((double)D.chr_cnt - 1.0));
}

// ---------------- sample blocks ----------------

// 10 kb blocks over twice the mean depth -> low-variance sample blocks
void lowvar_blocks(const grom_params &P, const unsigned long long hacc[4], const std::vector<int64_t> &blk_total,
                   int64_t len, std::vector<long> &ss, std::vector<long> &se) {
    const int64_t m = P.insert_mean, W = 2 * (int64_t)m - 1, n_blk = len / BLOCK_UNIT;
    const double chr_rd_ave = (double)hacc[0] / (double)hacc[1];
    const double chr_rd_thr = P.chr_rd_threshold_factor * chr_rd_ave;
    std::vector<long> over;
    for (int64_t b = 0; b < n_blk; b++)
        if (blk_total[b] / (double)BLOCK_UNIT > chr_rd_thr) over.push_back((long)b);
    std::vector<long> bs(MAX_BLOCK_LIST), be(MAX_BLOCK_LIST);
    long tb = 0, tbs = 0, tbe = 0, nbk = 0;
    for (size_t a = 1; a < over.size(); a++) {
        if (tb == 0) {
            if ((tb + 1) > ((over[a] - over[a - 1]) / BLOCK_FACTOR)) { tbe = over[a] + 1; tb += 1; }
            else tbe = over[a - 1] + 1;
            tbs = over[a - 1];
            tb += 1;
        } else {
            if ((tb + 1) > ((over[a - 1] - tbs) / BLOCK_FACTOR)) { tbe = over[a - 1] + 1; tb += 1; }
            else {
                if (tb >= P.min_blocks) nbk += 1;
                tb = 1;
                tbs = over[a - 1];
                tbe = over[a - 1] + 1;
            }
            if (tb >= P.min_blocks && nbk < MAX_BLOCK_LIST) {
                bs[nbk] = tbs * BLOCK_UNIT;
                be[nbk] = tbe * BLOCK_UNIT;
            }
        }
    }
    if (tb >= P.min_blocks) nbk += 1;
    std::vector<long> ls(1, 0), le;
    for (long a = 0; a < nbk && a < MAX_BLOCK_LIST; a++)
        if (be[a] - bs[a] >= P.block_min) { le.push_back(bs[a]); ls.push_back(be[a]); }
    le.push_back(len);
    for (size_t k = 0; k < ls.size(); k++) {
        for (long *v : {&ls[k], &le[k]}) {
            if (*v < m - 1) *v = m - 1;
            else if (*v >= len - W) *v = len - W;
        }
    }
    ss.clear();
    se.clear();
    for (size_t k = 0; k < ls.size(); k++)
        if (!(le[k] - ls[k] < P.min_rd_window_len)) { ss.push_back(ls[k]); se.push_back(le[k]); }
}

// ---------------- sampling ----------------

std::vector<GatherRange> bin_sample_ranges(const std::vector<long> &ss, const std::vector<long> &se, long half,
                                           int64_t *total) {
    std::vector<GatherRange> rg;
    int64_t tot = 0;
    for (size_t b = 0; b < ss.size(); b++) {
        if (se[b] <= ss[b] || half <= 0) continue;
        int64_t c = (se[b] - ss[b] + half - 1) / half;
        rg.push_back(GatherRange{ss[b], c, half, tot});
        tot += c;
    }
    *total = tot;
    return rg;
}

std::vector<GatherRange> repeat_ranges(const std::vector<RepeatRec> &reps, int biased, long half, int64_t *total) {
    std::vector<GatherRange> rrg;
    int64_t tot = 0;
    if (biased != -1)
        for (auto &r : reps)
            if (r.type == biased) {
                rrg.push_back(GatherRange{r.start - half, r.end - r.start + 2 * half, 1, tot});
                tot += r.end - r.start + 2 * half;
            }
    *total = tot;
    return rrg;
}

// the flank segment of a base of a gathered repeat [rs, re) +- half
static int repeat_segment(int64_t pos, int64_t rs, int64_t re, long half) {
    if (pos < rs) return (int)((REP_SEGS - 1) * (pos - (rs - half)) / half);
    if (pos >= re) return (int)((REP_SEGS - 1) * ((re + half) - pos) / half);
    return REP_SEGS - 1;
}

void sample_repeats(Reservoir &R, const std::vector<GatherRange> &rrg, long half, const GatherView &g,
                    RepeatSamples &out) {
    for (auto &x : rrg) {
        const int64_t rs = x.start + half, re = x.start + x.count - half;
        for (int64_t i = 0; i < x.count; i++) {
            const int64_t pos = x.start + i, o = x.out + i;
            if (g.ac[o] < MIN_ACGT) continue;
            const int seg = repeat_segment(pos, rs, re, half);
            R.push(out.smp[seg], out.idx[seg], out.all[seg], g.rt[o]);
        }
    }
}

void sample_bins(Reservoir &R, int64_t total, const GatherView &g, int rd_min_mapq, BinSamples &out) {
    int last_low = 0;
    for (int64_t i = 0; i < total; i++) {
        if (g.ac[i] < MIN_ACGT) continue;
        const int bin = g.gc[i], v = g.rt[i];
        int k;
        if (v == 0) k = last_low;
        else k = last_low = (g.mq[i] >= rd_min_mapq) ? 0 : 1;
        R.push(out.smp[k][bin], out.idx[k][bin], out.all[k][bin], v);
    }
    for (int k = 0; k < 2; k++)
        for (int b = 0; b < NBINS; b++) sort_depths(out.smp[k][b]);
}

// thin bins borrow their +-2 neighbours' samples
void borrow_thin_bins(BinSamples &B, long sample_cap) {
    for (int k = 0; k < 2; k++) {
        std::vector<std::vector<int>> add(NBINS);
        bool thin[NBINS];
        for (int b = 0; b < NBINS; b++)
            thin[b] = b >= 2 && b < NBINS - 2 && B.idx[k][b] >= RD_MIN_WINDOWS && B.idx[k][b] < NO_COMBINE;
        for (int b = 0; b < NBINS; b++) {
            if (!thin[b]) continue;
            long n = B.idx[k][b];
            for (int a = b - 2; a <= b + 2; a++)
                if (a != b)
                    for (long j = 0; j < B.idx[k][a] && n < sample_cap; j++, n++) add[b].push_back(B.smp[k][a][j]);
        }
        for (int b = 0; b < NBINS; b++)
            if (thin[b]) {
                B.smp[k][b].insert(B.smp[k][b].end(), add[b].begin(), add[b].end());
                B.idx[k][b] = (long)B.smp[k][b].size();
                sort_depths(B.smp[k][b]);
            }
    }
}

// (the squares below are written d * d: the library's host compiler turns
// pow(d, 2) into the same multiply, and a compiler that calls libm instead
// must not change a last bit)
void repeat_segment_stats(RepeatSamples &R) {
    for (int r = 0; r < REP_SEGS; r++) {
        std::sort(R.smp[r].begin(), R.smp[r].end());
        if (R.idx[r] > 0) {
            long s0 = R.idx[r] / 20, e0 = R.idx[r] - s0, n0 = e0 - s0;
            for (long a = s0; a < e0; a++) R.ave[r] += R.smp[r][a];
            R.ave[r] = R.ave[r] / n0;
            for (long a = s0; a < e0; a++) {
                const double d = R.smp[r][a] - R.ave[r];
                R.sd[r] += d * d;
            }
            if (n0 > 1) R.sd[r] = sqrt(R.sd[r] / (n0 - 1));
        }
    }
}

void bin_stats(const BinSamples &B, const grom_params &P, Tables &T, std::vector<int32_t> &flat) {
    const double del_f = (1.0 - PLOIDY_NUM / P.ploidy), dup_f = (1.0 + PLOIDY_NUM / P.ploidy);
    flat.clear();
    for (int k = 0; k < 2; k++)
        for (int b = 0; b < NBINS; b++) {
            const long n = B.idx[k][b];
            const std::vector<int> &l = B.smp[k][b];
            T.off[k][b] = (int32_t)flat.size();
            T.cnt[k][b] = (int32_t)n;
            flat.insert(flat.end(), l.begin(), l.end());
            if (n > 0) {
                double a = 0.0;
                for (long j = 0; j < n; j++) a += l[j];
                a = a / n;
                // the same sequential sum; the square evaluated once per run of equal depths
                double s = 0.0;
                for (long j = 0; j < n;) {
                    const int v = l[j];
                    const double d = v - a, term = d * d;
                    for (; j < n && l[j] == v; j++) s += term;
                }
                if (n > 1) s = sqrt(s / (n - 1));
                T.ave[k][b] = a;
                T.sdv[k][b] = s;
                T.thr[0][k][b] = del_f * a;
                T.thr[1][k][b] = dup_f * a;
                T.wins[k][b] = n;
            }
        }
}

// ---------------- p values ----------------

namespace {
constexpr double ERF_P = 0.3275911, ERF_A1 = 0.254829592, ERF_A2 = -0.284496736, ERF_A3 = 1.421413741,
                 ERF_A4 = -1.453152027, ERF_A5 = 1.061405429;
inline double erf_tail(double t, double x) {
    return 1.0 - ((ERF_A1 * t + ERF_A2 * (t * t) + ERF_A3 * pow(t, 3) + ERF_A4 * pow(t, 4) + ERF_A5 * pow(t, 5)) *
                  exp(-(x * x)));
}
}  // namespace

// pval2sd, find_disc_svs GROM.c:20705-20748: t = 1 / (1 + p x)
void pval2sd_table(Tables &T) {
    const double sd_max = 10.0;
    int n = (int)(sd_max / STDEV_STEP + 0.5) + 1;
    T.n_p2s = n;
    for (int k = 0; k < n; k++) {
        double s = sd_max - k * STDEV_STEP;
        if (s < 0) s = 0;
        double x = s / sqrt(2.0), t = 1.0 / (1.0 + ERF_P * x);
        T.p2s_p[k] = (1.0 - erf_tail(t, x)) / 2.0;
        T.p2s_sd[k] = s;
    }
}

// the row's p value, GROM.c:17139-17300: t = 1 / (1 + p + x), the reference's
// own (not the table's 1 + p x); kept as it is
double row_pvalue(double stdevs) {
    double x = fabs(stdevs) / sqrt(2.0);
    double t = 1.0 / (1.0 + ERF_P + x);
    return (1.0 - erf_tail(t, x)) / 2.0;
}

// ---------------- windows ----------------

WindowPlan window_plan(const std::vector<long> &ss, const std::vector<long> &se, const grom_params &P) {
    const int64_t L = P.max_rd_window_len, F = P.windows_sampling_factor, ML = P.min_rd_window_len;
    WindowPlan W;
    std::vector<WinDesc> &wds = W.wds;
    std::vector<WinPiece> &wps = W.wps;
    long twc = 0;  // ddd_temp_win_count carries across blocks
    for (size_t b = 0; b < ss.size(); b++) {
        std::vector<std::pair<int64_t, int64_t>> segs;  // (start, count) of each sampling pass
        for (int64_t s = 0; s < F; s++) {
            int64_t a = ss[b] + s * L / F;
            if (a < se[b]) segs.push_back({a, se[b] - a});
        }
        // chop the concatenation into windows of L
        size_t si = 0;
        int64_t so = 0;
        while (si < segs.size()) {
            WinDesc d{};
            int64_t need = L, got = 0;
            d.piece0 = (int64_t)wps.size();
            while (need > 0 && si < segs.size()) {
                int64_t take = std::min(need, segs[si].second - so);
                wps.push_back(WinPiece{segs[si].first + so, take});
                so += take;
                need -= take;
                got += take;
                if (so == segs[si].second) { si++; so = 0; }
            }
            d.n_pieces = (int64_t)wps.size() - d.piece0;
            d.ntot = got;
            {
                int64_t *pp[3] = {&d.p0, &d.p1, &d.p2}, *nn[3] = {&d.n0, &d.n1, &d.n2};
                for (int64_t q = 0; q < 3 && q < d.n_pieces; q++) {
                    *pp[q] = wps[(size_t)(d.piece0 + q)].start;
                    *nn[q] = wps[(size_t)(d.piece0 + q)].count;
                }
            }
            if (twc == 0 && got >= ML) {
                d.row = (int64_t)wds.size();
                wds.push_back(d);
                W.rlen.push_back(got);
            } else {
                wps.resize((size_t)d.piece0);  // not sampled: its pieces are not needed
            }
            if (got == L) { twc += 1; if (twc == REDUCTION) twc = 0; }
        }
    }
    return W;
}

std::vector<double> window_sd(const std::vector<double> &wtot, const std::vector<int64_t> &wcnt, int64_t ML, int64_t L) {
    std::vector<double> wsd(L + 1, 0.0);
    for (int64_t l = ML; l <= L; l++) wsd[l] = wcnt[l] > 1 ? sqrt(wtot[l] / (wcnt[l] - 1)) : 0.0;  // GROM.c:19162
    return wsd;
}

void window_sd_minima(const std::vector<double> &wsd, int64_t L, std::vector<double> &wmin,
                      std::vector<double> &wmin512) {
    wmin.assign((size_t)L + 2, 0.0);
    for (int64_t a = 0; a <= L; a++) {
        double v = wsd[a];
        for (int64_t b2 = a + 1; b2 <= std::min<int64_t>(a + 63, L); b2++) v = std::min(v, wsd[b2]);
        wmin[a] = v;
    }
    wmin[L + 1] = 0.0;
    // the same over 512 lengths (phase B's block skip), from the 64-length minima
    wmin512.assign((size_t)L + 2, 0.0);
    for (int64_t a = 0; a <= L; a++) {
        double v = wmin[a];
        for (int64_t b2 = a + 64; b2 <= std::min<int64_t>(a + 511, L); b2 += 64) v = std::min(v, wmin[b2]);
        wmin512[a] = v;
    }
}

// ---------------- repeat z override ----------------

void repeat_z_override(const std::vector<GatherRange> &rrg, long half, const GatherView &g, const RepeatSamples &R,
                       const Tables &T, const grom_params &P, double dup_factor, std::vector<int64_t> &up_p,
                       std::vector<double> &up_z) {
    const int64_t rt_ = rrg.empty() ? 0 : rrg.back().out + rrg.back().count;
    std::vector<double> zv(rt_);
    std::vector<int64_t> zp(rt_);
    int64_t nz = 0;
    for (auto &x : rrg) {
        const int64_t rs = x.start + half, re = x.start + x.count - half;
        for (int64_t i = 0; i < x.count; i++) {
            const int64_t pos = x.start + i, o = x.out + i;
            const int seg = repeat_segment(pos, rs, re, half);
            if (g.flag[o] & F_LOW) continue;
            const long n = R.idx[seg];
            const int *l = R.smp[seg].data();
            const int r = g.rt[o];
            const double ave = R.ave[seg], sdv = R.sd[seg];
            long i1, i2;
            double z;
            if (r < ave) {
                i1 = cnv_bisect_right(l, r, 0, n);
                i2 = cnv_bisect_left(l, r, 0, n);
                double d1 = (i1 <= 0) ? 0.5 : (double)i1, d2 = (i2 <= 0) ? 0.5 : (double)i2;
                i1 = cnv_bisect_right_double(T.p2s_p, (d1 + d2) / (2 * n), 0, T.n_p2s);
                if (i1 < 0) i1 = 0; else if (i1 >= T.n_p2s) i1 = T.n_p2s - 1;
                z = P.ranks_stdev == 0 ? (ave - g.rd[o] - g.low[o]) / sdv : T.p2s_sd[i1];
            } else {
                const bool ov = r > dup_factor * ave;
                if (ov) { i1 = cnv_bisect_left(l, (int)(dup_factor * ave), 0, n); i2 = cnv_bisect_right(l, r, 0, n); }
                else { i1 = cnv_bisect_left(l, r, 0, n); i2 = cnv_bisect_right(l, r, 0, n); }
                i1 = n - i1;
                i2 = n - i2;
                double d1 = (i1 <= 0) ? 0.5 : (double)i1, d2 = (i2 <= 0) ? 0.5 : (double)i2;
                i1 = cnv_bisect_right_double(T.p2s_p, (d1 + d2) / (2 * n), 0, T.n_p2s);
                if (i1 < 0) i1 = 0; else if (i1 >= T.n_p2s) i1 = T.n_p2s - 1;
                if (P.ranks_stdev == 0)
                    z = ov ? (dup_factor - 1) * (-ave) / sdv : (ave - g.rd[o] - g.low[o]) / sdv;
                else z = -T.p2s_sd[i1];
            }
            zp[nz] = pos;
            zv[nz] = z;
            nz++;
        }
    }
    // later writes win, as in the reference's loop order: keep each
    // position's last value
    std::vector<int64_t> ord(nz);
    for (int64_t i = 0; i < nz; i++) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](int64_t x, int64_t y) { return zp[x] < zp[y]; });
    up_p.clear();
    up_z.clear();
    up_p.reserve(nz);
    up_z.reserve(nz);
    for (int64_t k = 0; k < nz; k++) {
        const int64_t i = ord[k];
        if (k + 1 < nz && zp[ord[k + 1]] == zp[i]) continue;  // a later write to the same base wins
        up_p.push_back(zp[i]);
        up_z.push_back(zv[i]);
    }
}

// ---------------- rows ----------------

std::vector<KeptCall> keep_calls(const std::vector<CallRec> &calls, double pval_threshold) {
    std::vector<KeptCall> keep;
    for (size_t i = 0; i < calls.size(); i++) {
        const double pv = row_pvalue(calls[i].stdevs);
        if (pv < pval_threshold) keep.push_back({i, pv});
    }
    return keep;
}

std::vector<GatherRange> call_ranges(const std::vector<CallRec> &calls, const std::vector<KeptCall> &keep,
                                     int64_t *total) {
    std::vector<GatherRange> rg;
    int64_t tot = 0;
    for (auto &kp : keep) {
        const CallRec &c = calls[kp.idx];
        int64_t n = std::max<int64_t>(0, c.ce - c.p);
        rg.push_back(GatherRange{c.p, n, 1, tot});
        tot += n;
    }
    *total = tot;
    return rg;
}

// copy number of every kept call (GROM.c:20100-20160): independent per call,
// so host threads share them
unsigned copy_numbers(const double *ratios, const std::vector<GatherRange> &rg, int ploidy, std::vector<double> &cnv_cn,
                      std::vector<double> &cnv_cs) {
    cnv_cn.assign(rg.size(), -1.0);
    cnv_cs.assign(rg.size(), 0.0);
    auto cn_of = [&](size_t j, std::vector<double> &pl, std::vector<double> &tmp) {
        pl.clear();
        const double *v = ratios + rg[j].out;
        for (int64_t i = 0; i < rg[j].count; i++)
            if (v[i] < HUGE_VAL) pl.push_back(v[i]);  // (the reference's list, in base order)
        double cn = -1, cns = 0;
        const long pc = (long)pl.size();
        if (pc > 0) {
            tmp.resize(pc);
            msort_lo_par(pl.data(), pl.size(), tmp.data(), 3);
            long s0 = 0.1 * pc, e0 = pc - s0;
            double sum = 0.0;
            for (long i = s0; i < e0; i++) sum += pl[i];
            if (e0 - s0 > 0) {
                cn = (sum / (e0 - s0)) * ploidy;
                cns = 0;
                for (long i = 0; i < pc; i++) {
                    const double d = ploidy * pl[i] - cn;
                    cns += d * d;
                }
                cns = sqrt(cns / pc);
            }
        }
        cnv_cn[j] = cn;
        cnv_cs[j] = cns;
    };
    int64_t work = 0;
    for (size_t j = 0; j < rg.size(); j++) work += rg[j].count;
    const unsigned nt = (unsigned)std::min<int64_t>({(int64_t)8, (int64_t)rg.size(), 1 + work / 200000});
    std::atomic<size_t> next{0};
    auto worker = [&] {
        std::vector<double> pl, tmp;
        for (size_t j; (j = next.fetch_add(1)) < rg.size();) cn_of(j, pl, tmp);
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; t++) th.emplace_back(worker);
    worker();
    for (auto &t : th) t.join();
    return nt;
}

int64_t format_rows(std::string &rows, const grom_params &P, int kind, const char *chr_name,
                    const std::vector<CallRec> &calls, const std::vector<KeptCall> &keep,
                    const std::vector<double> &cn, const std::vector<double> &cs) {
    // -f: a column header before each kind's rows (GROM.c:17242-17245,
    // 17378), rows named by caf_del_text / caf_dup_text (GROM.c:1575)
    if (P.vcf != 1) rows += "SV Type\tChromosome\tStart\tEnd\tStdev from mean\tP Value\tCopy Number\n";
    for (size_t j = 0; j < keep.size(); j++) {
        const CallRec &c = calls[keep[j].idx];
        char line[512];
        int nl;
        if (P.vcf != 1)  // GROM.c:17340-17343
            nl = snprintf(line, sizeof(line), "%s\t%s\t%lld\t%lld\t%e\t%e\t%e\t%e\n", kind == 0 ? "DEL RD" : "DUP RD",
                          chr_name, (long long)c.p, (long long)c.ce, c.stdevs, keep[j].pv, cn[j], cs[j]);
        else
            nl = snprintf(line, sizeof(line), "%s\t%lld\t.\t.\t%s\t.\t.\tEND=%lld\tSD:Z:CN:CS\t%e:%e:%.2f:%e\n",
                          chr_name, (long long)c.p + 1, kind == 0 ? "<DEL>" : "<DUP>", (long long)c.ce + 1,
                          c.stdevs, keep[j].pv, cn[j], cs[j]);
        rows.append(line, (size_t)nl);
    }
    return (int64_t)keep.size();
}

// ---------------- test hook: recorded host inputs and outputs ----------------

namespace {
constexpr char CNVH_MAGIC[8] = {'G', 'C', 'N', 'H', '1', 0, 0, 0};
}

HostDump::HostDump(const char *chr_name) {
    const char *dir = getenv("GROM_CNV_HOST_DUMP");
    if (!dir || !*dir) return;
    const std::string path = std::string(dir) + "/" + chr_name + ".cnvh";
    f = fopen(path.c_str(), "wb");
    if (f) fwrite(CNVH_MAGIC, 1, 8, f);
}
HostDump::~HostDump() {
    if (f) fclose(f);
}
void HostDump::put(const char *tag, const void *p, size_t bytes) {
    if (!f) return;
    char t[16] = {0};
    snprintf(t, sizeof(t), "%s", tag);
    const uint64_t n = bytes;
    fwrite(t, 1, 16, f);
    fwrite(&n, 8, 1, f);
    if (bytes) fwrite(p, 1, bytes, f);
}

namespace {
struct Record {
    std::map<std::string, std::string> blobs;
    bool has(const char *tag) const { return blobs.count(tag) != 0; }
    const std::string &raw(const char *tag) const {
        static const std::string none;
        auto it = blobs.find(tag);
        return it == blobs.end() ? none : it->second;
    }
    template <class T>
    std::vector<T> vec(const char *tag) const {
        const std::string &b = raw(tag);
        std::vector<T> v(b.size() / sizeof(T));
        if (!v.empty()) memcpy(v.data(), b.data(), v.size() * sizeof(T));
        return v;
    }
    // one recorded output against what the replay computed
    int64_t differs(const char *tag, const void *p, size_t bytes) const {
        const std::string &b = raw(tag);
        const bool same = has(tag) && b.size() == bytes && (bytes == 0 || memcmp(b.data(), p, bytes) == 0);
        if (!same) fprintf(stderr, "cnvhost: %s differs\n", tag);
        return same ? 0 : 1;
    }
    template <class T>
    int64_t differs(const char *tag, const std::vector<T> &v) const { return differs(tag, v.data(), sizeof(T) * v.size()); }
};

bool read_record(const char *path, Record &R) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    char magic[8];
    bool ok = fread(magic, 1, 8, f) == 8 && memcmp(magic, CNVH_MAGIC, 8) == 0;
    while (ok) {
        char t[16];
        uint64_t n;
        if (fread(t, 1, 16, f) != 16) break;  // end of file
        t[15] = 0;
        ok = fread(&n, 8, 1, f) == 1 && n <= ((uint64_t)1 << 32);
        if (!ok) break;
        std::string b((size_t)n, '\0');
        ok = n == 0 || fread(&b[0], 1, (size_t)n, f) == n;
        R.blobs[t] = std::move(b);
    }
    fclose(f);
    return ok;
}
}  // namespace

}  // namespace cnvcall

extern "C" int64_t grom_cnv_host_replay(const char *path) {
    using namespace cnvcall;
    Record R;
    if (!read_record(path, R)) return -1;
    if (R.raw("params").size() != sizeof(grom_params) || R.raw("seed").size() != 4 || R.raw("len").size() != 8 ||
        R.raw("hacc").size() != 32 || R.raw("sample_len").size() != 8)
        return -2;
    grom_params P;
    memcpy(&P, R.raw("params").data(), sizeof(P));
    uint32_t seed;
    int64_t len;
    long cap;
    unsigned long long hacc[4];
    memcpy(&seed, R.raw("seed").data(), 4);
    memcpy(&len, R.raw("len").data(), 8);
    memcpy(&cap, R.raw("sample_len").data(), 8);
    memcpy(hacc, R.raw("hacc").data(), 32);
    const std::string chr = R.raw("chr");
    const long half = P.insert_mean / 2;
    int64_t bad = 0;

    // depth statistics, the biased repeat, the sample blocks
    const std::vector<RepeatRec> reps = R.vec<RepeatRec>("reps");
    const DepthStats D = depth_stats(hacc, reps);
    int biased = -1;
    if (R.has("serial_rd")) {  // the run took the serial sum (forced, or the bound undecided)
        const std::vector<int32_t> rd = R.vec<int32_t>("serial_rd"), low = R.vec<int32_t>("serial_low");
        const std::vector<uint8_t> acw = R.vec<uint8_t>("serial_acw");
        if (low.size() != rd.size() || acw.size() != rd.size()) return -2;
        biased = biased_repeat(D, P, depth_sd_serial(D, rd.data(), low.data(), acw.data(), (int64_t)rd.size()));
    } else if (!biased_repeat_from_hist(D, P, R.vec<unsigned int>("hist"), &biased)) {
        fprintf(stderr, "cnvhost: histogram bound undecided, no serial arrays recorded\n");
        return -3;
    }
    bad += R.differs("biased", &biased, 4);
    std::vector<long> ss, se;
    lowvar_blocks(P, hacc, R.vec<int64_t>("blk_total"), len, ss, se);
    bad += R.differs("ss", ss) + R.differs("se", se);

    // sampling -> Tables and the flat sample array
    Reservoir res(seed, cap);
    int64_t tot = 0, rtot = 0;
    const std::vector<GatherRange> rg = bin_sample_ranges(ss, se, half, &tot);
    const std::vector<GatherRange> rrg = repeat_ranges(reps, biased, half, &rtot);
    const std::vector<uint8_t> g_ac = R.vec<uint8_t>("g_ac"), g_gc = R.vec<uint8_t>("g_gc");
    const std::vector<int32_t> g_rt = R.vec<int32_t>("g_rt"), g_mq = R.vec<int32_t>("g_mq");
    const std::vector<uint8_t> r_ac = R.vec<uint8_t>("r_ac");
    const std::vector<int32_t> r_rt = R.vec<int32_t>("r_rt");
    if ((int64_t)g_ac.size() != tot || (int64_t)g_gc.size() != tot || (int64_t)g_rt.size() != tot ||
        (int64_t)g_mq.size() != tot || (int64_t)r_ac.size() != rtot || (int64_t)r_rt.size() != rtot)
        return -4;
    RepeatSamples RS;
    BinSamples BS;
    GatherView gv, rv;
    gv.ac = g_ac.data(), gv.gc = g_gc.data(), gv.rt = g_rt.data(), gv.mq = g_mq.data();
    rv.ac = r_ac.data(), rv.rt = r_rt.data();
    if (biased != -1) sample_repeats(res, rrg, half, rv, RS);
    sample_bins(res, tot, gv, (int)P.rd_min_mapq, BS);
    const long draws[2] = {res.over, res.repl};
    bad += R.differs("draws", draws, sizeof(draws));
    borrow_thin_bins(BS, cap);
    if (biased != -1) repeat_segment_stats(RS);
    Tables *T = new Tables();  // (value-initialised: the padding is compared too)
    std::vector<int32_t> flat;
    bin_stats(BS, P, *T, flat);
    pval2sd_table(*T);
    bad += R.differs("tables", T, TABLES_BYTES) + R.differs("samples", flat);

    // the window plan, wsd and its minima
    const WindowPlan WP = window_plan(ss, se, P);
    bad += R.differs("wds", WP.wds) + R.differs("wps", WP.wps) + R.differs("rlen", WP.rlen);
    const int64_t L = P.max_rd_window_len, ML = P.min_rd_window_len;
    const std::vector<double> wtot = R.vec<double>("wtot");
    const std::vector<int64_t> wcnt = R.vec<int64_t>("wcnt");
    if ((int64_t)wtot.size() != L + 1 || (int64_t)wcnt.size() != L + 1) {
        delete T;
        return -4;
    }
    const std::vector<double> wsd = window_sd(wtot, wcnt, ML, L);
    std::vector<double> wmin, wmin512;
    window_sd_minima(wsd, L, wmin, wmin512);
    bad += R.differs("wsd", wsd) + R.differs("wmin", wmin) + R.differs("wmin512", wmin512);

    // the repeat z override
    if (biased != -1 && !rrg.empty()) {
        const std::vector<uint8_t> o_flag = R.vec<uint8_t>("o_flag");
        const std::vector<int32_t> o_rt = R.vec<int32_t>("o_rt"), o_rd = R.vec<int32_t>("o_rd"),
                                   o_low = R.vec<int32_t>("o_low");
        if ((int64_t)o_flag.size() != rtot || (int64_t)o_rt.size() != rtot || (int64_t)o_rd.size() != rtot ||
            (int64_t)o_low.size() != rtot) {
            delete T;
            return -4;
        }
        GatherView ov;
        ov.flag = o_flag.data(), ov.rt = o_rt.data(), ov.rd = o_rd.data(), ov.low = o_low.data();
        std::vector<int64_t> zp;
        std::vector<double> zv;
        repeat_z_override(rrg, half, ov, RS, *T, P, (double)P.dup_threshold_factor, zp, zv);
        bad += R.differs("zover_pos", zp) + R.differs("zover_z", zv);
    }
    delete T;

    // rows of both kinds (the threaded copy-number step)
    std::string rows;
    for (int kind = 0; kind < 2; kind++) {
        const std::vector<CallRec> calls = R.vec<CallRec>(kind == 0 ? "calls0" : "calls1");
        const std::vector<double> ratios = R.vec<double>(kind == 0 ? "ratios0" : "ratios1");
        const std::vector<KeptCall> keep = keep_calls(calls, P.rd_pval_threshold);
        int64_t ctot = 0;
        const std::vector<GatherRange> crg = call_ranges(calls, keep, &ctot);
        if ((int64_t)ratios.size() != ctot) return -4;
        std::vector<double> cn, cs;
        copy_numbers(ratios.data(), crg, (int)P.ploidy, cn, cs);
        format_rows(rows, P, kind, chr.c_str(), calls, keep, cn, cs);
    }
    bad += R.differs("rows", rows.data(), rows.size());
    return bad;
}

// ---- test hooks (tests/test_oracle_cnv.py) ----
extern "C" void grom_cnv_test_rand(uint32_t seed, int n, int32_t *out) {
    cnvcall::GlibcRand g(seed);
    for (int i = 0; i < n; i++) out[i] = g.next();
}
extern "C" void grom_cnv_test_msort_lo(double *v, int64_t n) {
    std::vector<double> t((size_t)std::max<int64_t>(n, 1));
    cnvcall::msort_lo(v, (size_t)n, t.data());
}
extern "C" long grom_cnv_test_bisect(int which, const int *l, const double *ld, long n, double v) {
    if (which == 0) return cnv_bisect_left(l, (int)v, 0, n);
    if (which == 1) return cnv_bisect_right(l, (int)v, 0, n);
    return cnv_bisect_right_double(ld, v, 0, n);
}
