// vcfsort.hip -- a VCF written position-sorted, bgzipped and tabix-indexed
// on the device: grom_vcf_writer_* and grom_vcf_tabix.
// device = -1 runs the host twin (vcfsort_host.cpp), which writes the same
// three files byte for byte.
//
// The writer collects the stream in pinned chunks; the sort is global (the
// CTX file's contigs interleave), so everything happens at close:
//   lines    k_vs_count / k_vs_starts   newlines per 4 KB tile, a prefix sum, the line starts
//   facts    k_vs_facts                 one lane per line: POS, beg0, end0 (vcfsort.h), header lines,
//                                       the rows whose CHROM differs from the row before
//            k_vs_heads                 the prefix sum of those flags names the runs; the host maps
//                                       the runs' names to contig ids in order of first appearance
//   sort     k_vs_keys                  (contig id << 32) | POS, the inversions, the bits that vary;
//                                       a stable LSD radix sort over the digits that vary, carrying the row
//   gather   k_vs_len / k_vs_gather     the sorted rows' lengths, a prefix sum, 16 lanes per row with
//                                       16-byte stores aligned on the destination
//   (the sorted text goes back to the pinned chunks and through grom_bgzf_writer_*)
//   index    k_vs_index / k_vs_runs /   virtual offsets from the writer's block offsets, bins, the runs of
//            k_vs_linear                one (contig, bin) in file order, the 16 kb windows' minima
// and the host feeds the runs to the BAI accumulator (vs_write_tbi).  One
// stream; every device buffer is a DevBuf freed at close.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/grom_amd.h"
#include "bgzfwrite.h"
#include "devbuf.h"
#include "vcfsort.h"
#include "vcfsort_host.h"

namespace {

using VBuf = DevBufOf<GROM_DEVCAT_OTHER, 256>;

#define VS_TPB 256
#define VS_TILE 4096  // the line kernels' bytes per workgroup: 16 per lane
#define VS_SUB 16     // the gather's lanes per row

// what the facts kernel reports: the first line that is a row, the last '#' line (+ 1; 0 none), a refused row
struct VsStat {
    unsigned long long first_row, last_hash1;
    unsigned int bad, pad;
    unsigned long long diff, inv;
};

__device__ __forceinline__ uint32_t vs_newlines(const uint4 v, int valid, uint32_t &mask) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    mask = 0;
#pragma unroll
    for (int k = 0; k < 16; k++)
        if (k < valid && ((w[k >> 2] >> (8 * (k & 3))) & 0xff) == '\n') mask |= 1u << k;
    return (uint32_t)__popc(mask);
}

// ---- the newlines of every 4 KB tile ----
__global__ void __launch_bounds__(VS_TPB) k_vs_count(const uint8_t *__restrict__ text, int64_t n,
                                                     uint32_t *__restrict__ tile_cnt) {
    typedef hipcub::BlockReduce<uint32_t, VS_TPB> Red;
    __shared__ typename Red::TempStorage tmp;
    const int64_t o = (int64_t)blockIdx.x * VS_TILE + (int64_t)threadIdx.x * 16;
    uint32_t c = 0, mask;
    if (o < n) c = vs_newlines(*reinterpret_cast<const uint4 *>(text + o), n - o < 16 ? (int)(n - o) : 16, mask);
    const uint32_t s = Red(tmp).Sum(c);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s;
}

// ---- ls[0] = 0, ls[k + 1] = the byte after newline k ----
__global__ void __launch_bounds__(VS_TPB) k_vs_starts(const uint8_t *__restrict__ text, int64_t n,
                                                      const uint32_t *__restrict__ tile_base, int64_t L,
                                                      int64_t *__restrict__ ls) {
    typedef hipcub::BlockScan<uint32_t, VS_TPB> Scan;
    __shared__ typename Scan::TempStorage tmp;
    const int64_t o = (int64_t)blockIdx.x * VS_TILE + (int64_t)threadIdx.x * 16;
    uint32_t c = 0, mask = 0, pre;
    if (o < n) c = vs_newlines(*reinterpret_cast<const uint4 *>(text + o), n - o < 16 ? (int)(n - o) : 16, mask);
    Scan(tmp).ExclusiveSum(c, pre);
    int64_t at = 1 + (int64_t)tile_base[blockIdx.x] + pre;
    for (; mask; mask &= mask - 1, at++)
        if (at <= L) ls[at] = o + (__ffs(mask) - 1) + 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) ls[0] = 0;
}

// ---- one lane per line: the row's facts, the header's end, the contig runs' heads ----
__global__ void __launch_bounds__(VS_TPB) k_vs_facts(const uint8_t *__restrict__ text, int64_t n,
                                                     const int64_t *__restrict__ ls, int64_t L, uint32_t *__restrict__ pos,
                                                     int32_t *__restrict__ beg, int32_t *__restrict__ end,
                                                     uint32_t *__restrict__ flag, VsStat *__restrict__ st) {
    const int64_t i = (int64_t)blockIdx.x * VS_TPB + threadIdx.x;
    if (i >= L) return;
    const int64_t a = ls[i], b = ls[i + 1];
    uint32_t fl = 0;
    VsFacts f;
    f.pos = 0, f.beg0 = 0, f.end0 = 1, f.err = VS_OK;
    if (a < 0 || b <= a || b > n) {
        atomicOr(&st->bad, 1u << 7);
    } else if (text[a] == '#') {
        atomicMax(&st->last_hash1, (unsigned long long)i + 1);
    } else {
        atomicMin(&st->first_row, (unsigned long long)i);
        f = vs_facts(text, a, b);
        if (f.err != VS_OK) atomicOr(&st->bad, 1u << f.err);
        fl = 1;
        if (i > 0) {
            const int64_t pa = ls[i - 1];
            if (pa >= 0 && pa < a && text[pa] != '#' && vs_same_chrom(text, pa, a, n)) fl = 0;
        }
    }
    pos[i] = f.pos;
    beg[i] = f.beg0;
    end[i] = f.end0;
    flag[i] = fl;
}

// rid = the inclusive sum of flag: the run a row belongs to (+ 1)
__global__ void __launch_bounds__(VS_TPB) k_vs_heads(const int64_t *__restrict__ ls, int64_t L,
                                                     const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rid,
                                                     int64_t n_runs, int64_t *__restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * VS_TPB + threadIdx.x;
    if (i >= L || !flag[i]) return;
    const int64_t r = (int64_t)rid[i] - 1;
    if (r >= 0 && r < n_runs) head[r] = ls[i];
}

__device__ __forceinline__ uint64_t vs_row_key(int64_t line, const uint32_t *rid, const uint32_t *run_cid, int64_t n_runs,
                                               const uint32_t *pos) {
    const int64_t r = (int64_t)rid[line] - 1;
    return vs_key(r >= 0 && r < n_runs ? run_cid[r] : 0u, pos[line]);
}

// ---- the keys, the row indices, the inversions, the bits in which the keys differ ----
__global__ void __launch_bounds__(VS_TPB) k_vs_keys(int64_t H, int64_t R, const uint32_t *__restrict__ rid,
                                                    const uint32_t *__restrict__ run_cid, int64_t n_runs,
                                                    const uint32_t *__restrict__ pos, uint64_t *__restrict__ key,
                                                    uint32_t *__restrict__ idx, VsStat *__restrict__ st) {
    const int64_t i = (int64_t)blockIdx.x * VS_TPB + threadIdx.x;
    uint64_t d = 0;
    bool inv = false;
    if (i < R) {
        const uint64_t k = vs_row_key(H + i, rid, run_cid, n_runs, pos);
        key[i] = k;
        idx[i] = (uint32_t)i;
        d = k ^ vs_row_key(H, rid, run_cid, n_runs, pos);
        inv = i > 0 && k < vs_row_key(H + i - 1, rid, run_cid, n_runs, pos);
    }
    uint32_t lo = (uint32_t)d, hi = (uint32_t)(d >> 32);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        lo |= (uint32_t)__shfl_xor((int)lo, s, 64);
        hi |= (uint32_t)__shfl_xor((int)hi, s, 64);
    }
    const unsigned long long ninv = (unsigned long long)__popcll(__ballot(inv));
    if ((threadIdx.x & 63) == 0) {
        const unsigned long long dd = ((unsigned long long)hi << 32) | lo;
        if (dd) atomicOr(&st->diff, dd);
        if (ninv) atomicAdd(&st->inv, ninv);
    }
}

// ---- len[j] = the bytes of sorted row j; len[R] = 0 ----
__global__ void __launch_bounds__(VS_TPB) k_vs_len(const int64_t *__restrict__ ls, int64_t H, int64_t R,
                                                   const uint32_t *__restrict__ perm, int64_t *__restrict__ len) {
    const int64_t j = (int64_t)blockIdx.x * VS_TPB + threadIdx.x;
    if (j > R) return;
    int64_t v = 0;
    if (j < R && (int64_t)perm[j] < R) {
        const int64_t line = H + perm[j];
        v = ls[line + 1] - ls[line];
    }
    len[j] = v;
}

// ---- the rows copied to their places: VS_SUB lanes per row, 16-byte stores aligned on dst ----
__global__ void __launch_bounds__(VS_TPB) k_vs_gather(const uint8_t *__restrict__ text, int64_t n,
                                                      const int64_t *__restrict__ ls, int64_t H, int64_t R,
                                                      const uint32_t *__restrict__ perm, const int64_t *__restrict__ doff,
                                                      int64_t hb, uint8_t *__restrict__ dst, int64_t dst_cap) {
    const uint32_t sub = threadIdx.x & (VS_SUB - 1);
    const int64_t j = ((int64_t)blockIdx.x * VS_TPB + threadIdx.x) / VS_SUB;
    if (j >= R || (int64_t)perm[j] >= R) return;
    const int64_t line = H + perm[j], S = ls[line], len = ls[line + 1] - S, D = hb + doff[j];
    if (S < 0 || len <= 0 || S + len > n || D < 0 || D + len > dst_cap) return;
    int64_t head = (0 - D) & 15;
    if (head > len) head = len;
    if ((int64_t)sub < head) dst[D + sub] = text[S + sub];
    const int64_t nw = (len - head) >> 4, s0 = S + head;
    const uint32_t a = (uint32_t)(s0 & 15), ws = a >> 2, bs = 8 * (a & 3);
    const uint4 *sw = reinterpret_cast<const uint4 *>(text + (s0 - a));  // (the text has 64 spare bytes)
    uint4 *dw = reinterpret_cast<uint4 *>(dst + D + head);
    for (int64_t k = sub; k < nw; k += VS_SUB) {
        // the source bytes [s0 + 16 k, s0 + 16 k + 16) out of two aligned words
        const uint4 lo = sw[k], hi = a ? sw[k + 1] : lo;
        const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        uint32_t r[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (uint32_t q = 0; q < 4; q++)
            if (q == ws) {
#pragma unroll
                for (int i = 0; i < 5; i++) r[i] = w[q + i];
            }
        uint4 v;
        v.x = bs ? (r[0] >> bs) | (r[1] << (32 - bs)) : r[0];
        v.y = bs ? (r[1] >> bs) | (r[2] << (32 - bs)) : r[1];
        v.z = bs ? (r[2] >> bs) | (r[3] << (32 - bs)) : r[2];
        v.w = bs ? (r[3] >> bs) | (r[4] << (32 - bs)) : r[3];
        dw[k] = v;
    }
    for (int64_t i = head + 16 * nw + sub; i < len; i += VS_SUB) dst[D + i] = text[S + i];
}

// a contig's rows in the sorted file, as the device finds them
struct VsDevSpan {
    uint64_t beg, end;
    int64_t j0, j1;
};

// ---- one lane per sorted row: virtual offsets, bin, run heads, the contigs' spans and window counts ----
__global__ void __launch_bounds__(VS_TPB) k_vs_index(int64_t H, int64_t R, int64_t L, const uint32_t *__restrict__ perm,
                                                     const uint64_t *__restrict__ ks, const int32_t *__restrict__ beg,
                                                     const int32_t *__restrict__ end, const int64_t *__restrict__ doff,
                                                     int64_t hb, const int64_t *__restrict__ coff, int64_t n_blk,
                                                     int64_t total, int32_t C, uint64_t *__restrict__ vbeg,
                                                     uint64_t *__restrict__ vend, uint32_t *__restrict__ bin,
                                                     uint32_t *__restrict__ hf, int32_t *__restrict__ maxw,
                                                     VsDevSpan *__restrict__ span) {
    const int64_t j = (int64_t)blockIdx.x * VS_TPB + threadIdx.x;
    if (j >= R) return;
    const int64_t line = H + perm[j];
    const int32_t c = (int32_t)(ks[j] >> 32);
    if (line >= L || c < 0 || c >= C) {
        vbeg[j] = vend[j] = 0;
        bin[j] = 0;
        hf[j] = 0;
        return;
    }
    const int32_t b0 = beg[line], e0 = end[line];
    const uint32_t bn = vs_reg2bin(b0, e0);
    const uint64_t vb = vs_voff(coff, n_blk, total, hb + doff[j]), ve = vs_voff(coff, n_blk, total, hb + doff[j + 1]);
    bool first = j == 0, head = j == 0;
    if (j > 0) {
        const int64_t pl = H + perm[j - 1];
        first = (int32_t)(ks[j - 1] >> 32) != c;
        head = first || pl >= L || vs_reg2bin(beg[pl], end[pl]) != bn;
    }
    const bool last = j == R - 1 || (int32_t)(ks[j + 1] >> 32) != c;
    vbeg[j] = vb;
    vend[j] = ve;
    bin[j] = bn;
    hf[j] = head ? 1u : 0u;
    // the contig's windows: a row whose successor in the contig reaches at least as far adds nothing (the
    // last row that reaches farthest has no such successor), which spares the one address nearly every atomic
    bool dominated = false;
    if (!last) {
        const int64_t nl = H + perm[j + 1];
        dominated = nl < L && end[nl] >= e0;
    }
    if (!dominated) atomicMax(&maxw[c], ((e0 - 1) >> 14) + 1);
    if (first) { span[c].beg = vb; span[c].j0 = j; }
    if (last) { span[c].end = ve; span[c].j1 = j; }
}

// rinc = the inclusive sum of hf: the run a sorted row belongs to (+ 1)
__global__ void __launch_bounds__(VS_TPB) k_vs_runs(int64_t R, const uint64_t *__restrict__ ks,
                                                    const uint32_t *__restrict__ bin, const uint64_t *__restrict__ vbeg,
                                                    const uint64_t *__restrict__ vend, const uint32_t *__restrict__ hf,
                                                    const uint32_t *__restrict__ rinc, VsRun *__restrict__ runs,
                                                    int64_t n_runs) {
    const int64_t j = (int64_t)blockIdx.x * VS_TPB + threadIdx.x;
    if (j >= R) return;
    const int64_t r = (int64_t)rinc[j] - 1;
    if (r < 0 || r >= n_runs) return;
    if (hf[j]) {
        runs[r].cid = (int32_t)(ks[j] >> 32);
        runs[r].bin = bin[j];
        runs[r].beg = vbeg[j];
    }
    if (j == R - 1 || hf[j + 1]) runs[r].end = vend[j];
}

// ---- the linear index: the smallest offset of a row over each 16 kb window ----
__global__ void __launch_bounds__(VS_TPB) k_vs_linear(int64_t H, int64_t R, int64_t L, const uint32_t *__restrict__ perm,
                                                      const uint64_t *__restrict__ ks, const int32_t *__restrict__ beg,
                                                      const int32_t *__restrict__ end, const uint64_t *__restrict__ vbeg,
                                                      const int64_t *__restrict__ lin_base, int32_t C,
                                                      unsigned long long *__restrict__ lin) {
    const int64_t j = (int64_t)blockIdx.x * VS_TPB + threadIdx.x;
    if (j >= R) return;
    const int64_t line = H + perm[j];
    const int32_t c = (int32_t)(ks[j] >> 32);
    if (line >= L || c < 0 || c >= C) return;
    const int32_t w0 = beg[line] >> 14, w1 = (end[line] - 1) >> 14;
    int32_t pw0 = 0, pw1 = -1;  // the row before covers these with a smaller offset
    if (j > 0 && (int32_t)(ks[j - 1] >> 32) == c) {
        const int64_t pl = H + perm[j - 1];
        if (pl < L) { pw0 = beg[pl] >> 14; pw1 = (end[pl] - 1) >> 14; }
    }
    const int64_t lb = lin_base[c], cap = lin_base[c + 1] - lb;
    const unsigned long long vb = vbeg[j];
    for (int32_t w = w0; w <= w1; w++) {
        if (w >= pw0 && w <= pw1) continue;
        if (w >= cap) break;
        atomicMin(&lin[lb + w], vb);
    }
}

#define VSK(x)                                                                                                  \
    do {                                                                                                        \
        hipError_t e_ = (x);                                                                                    \
        if (e_ != hipSuccess) {                                                                                 \
            snprintf(err, sizeof(err), "VCF sort: HIP error %s at %s:%d", hipGetErrorString(e_), __FILE__, __LINE__); \
            return GROM_E_HIP;                                                                                  \
        }                                                                                                       \
    } while (0)
#define VSG(b, bytes)                                                                             \
    do {                                                                                          \
        if ((b).grow(bytes)) {                                                                    \
            snprintf(err, sizeof(err), "VCF sort: hipMalloc(%lld) failed", (long long)(bytes));   \
            return GROM_E_NOMEM;                                                                  \
        }                                                                                         \
    } while (0)

// the writer's device for the length of a call: the caller's current device is put back
struct DevGuard {
    int prev = -1;
    bool ok;
    explicit DevGuard(int d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(d) == hipSuccess;
    }
    ~DevGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

unsigned blocks_for(int64_t items) { return (unsigned)std::max<int64_t>(1, (items + VS_TPB - 1) / VS_TPB); }

int64_t chunk_bytes() {
    const char *e = getenv("GROM_VCF_CHUNK_KB");
    int64_t b = (int64_t)32 << 20;
    if (e && atof(e) > 0) b = (int64_t)(atof(e) * 1024.0);
    return std::max<int64_t>(b, 1024);
}

}  // namespace

struct grom_vcf_writer {
    std::string path;
    int device = -1;
    int64_t chunk = 0, n = 0;
    std::vector<uint8_t *> chunks;  // pinned with a device, else malloc
    hipStream_t st = nullptr;
    hipEvent_t ev[6] = {};
    VBuf text, sorted, tile_cnt, tile_base, tmp, ls, pos, beg, end, flag, rid, head, run_cid, key, key2, idx, idx2, len, doff,
        stat, coff, vbeg, vend, bin, hf, rinc, runs, maxw, span, lin_base, lin;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    int failed = 0;
    char err[4600] = {0};

    int fail(int code, const char *m) {
        if (!failed) {
            failed = code;
            if (m != err) snprintf(err, sizeof(err), "%s", m);
        }
        return failed;
    }
    uint8_t *chunk_alloc() {
        uint8_t *p = nullptr;
        if (device >= 0) {
            DevGuard g(device);
            if (hipHostMalloc((void **)&p, (size_t)chunk, hipHostMallocDefault) != hipSuccess) p = nullptr;
        } else {
            p = (uint8_t *)malloc((size_t)chunk);
        }
        return p;
    }
    void free_all() {
        if (device >= 0) {
            DevGuard g(device);
            if (st) (void)hipStreamSynchronize(st);
            for (hipEvent_t &e : ev)
                if (e) { (void)hipEventDestroy(e); e = nullptr; }
            if (st) (void)hipStreamDestroy(st);
            st = nullptr;
            for (VBuf *b : {&text, &sorted, &tile_cnt, &tile_base, &tmp, &ls, &pos, &beg, &end, &flag, &rid, &head, &run_cid,
                            &key, &key2, &idx, &idx2, &len, &doff, &stat, &coff, &vbeg, &vend, &bin, &hf, &rinc, &runs, &maxw,
                            &span, &lin_base, &lin})
                b->release();
            for (uint8_t *p : chunks) (void)hipHostFree(p);
        } else {
            for (uint8_t *p : chunks) free(p);
        }
        chunks.clear();
    }
    // where the stream's next byte goes and how many fit there (a new chunk when the last is full); NULL: failed
    uint8_t *room(int64_t *avail) {
        const int64_t at = n % chunk;
        if ((int64_t)chunks.size() * chunk == n) {
            uint8_t *c = chunk_alloc();
            if (!c) {
                fail(GROM_E_NOMEM, "VCF sort: out of host memory");
                return nullptr;
            }
            chunks.push_back(c);
        }
        *avail = chunk - at;
        return chunks.back() + at;
    }
    // the collected stream as one block of host memory (the host twin, and the wording of a refusal)
    std::vector<uint8_t> contiguous() const {
        std::vector<uint8_t> all((size_t)n + 1);
        for (int64_t o = 0; o < n; o += chunk) memcpy(all.data() + o, chunks[(size_t)(o / chunk)], (size_t)std::min(chunk, n - o));
        return all;
    }
    float ms(int a, int b) {
        float v = 0;
        return hipEventElapsedTime(&v, ev[a], ev[b]) == hipSuccess ? v : 0.0f;
    }
    int scan_u32(uint32_t *in, uint32_t *out, int64_t items, bool inclusive);
    int run_device(int64_t out[12]);
};

// the sum of `items` uint32 on the stream (hipcub's scan; its scratch in tmp)
int grom_vcf_writer::scan_u32(uint32_t *in, uint32_t *out, int64_t items, bool inclusive) {
    size_t tb = 0;
    if (inclusive) VSK(hipcub::DeviceScan::InclusiveSum(nullptr, tb, in, out, (int)items, st));
    else VSK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, (int)items, st));
    if (tmp.cap < tb) {
        VSK(hipStreamSynchronize(st));  // (the scratch may still be read)
        VSG(tmp, tb);
    }
    if (inclusive) VSK(hipcub::DeviceScan::InclusiveSum(tmp.p, tb, in, out, (int)items, st));
    else VSK(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, in, out, (int)items, st));
    return 0;
}

int grom_vcf_writer::run_device(int64_t out[12]) {
    DevGuard g(device);
    if (n > 0 && chunks[(size_t)((n - 1) / chunk)][(n - 1) % chunk] != '\n') return fail(GROM_E_ARG, VS_MSG_NO_NEWLINE);
    const int64_t ntile = (n + VS_TILE - 1) / VS_TILE;
    if (ntile + 1 > 0x7fffffff) return fail(GROM_E_ARG, "VCF sort: the stream is too long");
    // ---- lines ----
    VSG(text, (size_t)n + 64);
    VSG(tile_cnt, sizeof(uint32_t) * (size_t)(ntile + 1));
    VSG(tile_base, sizeof(uint32_t) * (size_t)(ntile + 1));
    VSG(stat, sizeof(VsStat));
    for (int64_t o = 0; o < n; o += chunk)
        VSK(hipMemcpyAsync(P<uint8_t>(text) + o, chunks[(size_t)(o / chunk)], (size_t)std::min(chunk, n - o),
                           hipMemcpyHostToDevice, st));
    VSK(hipEventRecord(ev[0], st));
    VSK(hipMemsetAsync(tile_cnt.p, 0, sizeof(uint32_t) * (size_t)(ntile + 1), st));
    if (ntile) hipLaunchKernelGGL(k_vs_count, dim3((unsigned)ntile), dim3(VS_TPB), 0, st, P<uint8_t>(text), n, P<uint32_t>(tile_cnt));
    int rc = scan_u32(P<uint32_t>(tile_cnt), P<uint32_t>(tile_base), ntile + 1, false);
    if (rc) return rc;
    uint32_t L32 = 0;
    VSK(hipMemcpyAsync(&L32, P<uint32_t>(tile_base) + ntile, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    VSK(hipStreamSynchronize(st));
    const int64_t L = (int64_t)L32;
    if (L >= 0x7fffffff) return fail(GROM_E_ARG, "VCF sort: too many lines");
    VSG(ls, sizeof(int64_t) * (size_t)(L + 2));
    for (VBuf *b : {&pos, &beg, &end, &flag, &rid}) VSG(*b, 4 * (size_t)(L + 1));
    if (ntile)
        hipLaunchKernelGGL(k_vs_starts, dim3((unsigned)ntile), dim3(VS_TPB), 0, st, P<uint8_t>(text), n, P<uint32_t>(tile_base), L,
                           P<int64_t>(ls));
    else
        VSK(hipMemsetAsync(ls.p, 0, sizeof(int64_t), st));
    // ---- facts ----
    VsStat hs;
    memset(&hs, 0, sizeof(hs));
    hs.first_row = (unsigned long long)L;
    VSK(hipMemcpyAsync(stat.p, &hs, sizeof(hs), hipMemcpyHostToDevice, st));
    int64_t n_runs = 0;
    if (L > 0) {
        hipLaunchKernelGGL(k_vs_facts, dim3(blocks_for(L)), dim3(VS_TPB), 0, st, P<uint8_t>(text), n, P<int64_t>(ls), L,
                           P<uint32_t>(pos), P<int32_t>(beg), P<int32_t>(end), P<uint32_t>(flag), P<VsStat>(stat));
        if ((rc = scan_u32(P<uint32_t>(flag), P<uint32_t>(rid), L, true)) != 0) return rc;
        uint32_t nr = 0;
        VSK(hipMemcpyAsync(&nr, P<uint32_t>(rid) + (L - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        VSK(hipMemcpyAsync(&hs, stat.p, sizeof(hs), hipMemcpyDeviceToHost, st));
        VSK(hipGetLastError());
        VSK(hipStreamSynchronize(st));
        n_runs = (int64_t)nr;
    } else {
        VSK(hipStreamSynchronize(st));
    }
    const int64_t H = (int64_t)hs.first_row, R = L - H;
    if (hs.bad || (int64_t)hs.last_hash1 > H) {
        // the first refused line and its message, worded by the host's loop over the same checks
        const std::vector<uint8_t> all = contiguous();
        if (vs_first_refusal(all.data(), n, err, sizeof(err))) return fail(GROM_E_ARG, err);
        return fail(GROM_E_HIP, "VCF sort: the device refused a stream that the host accepts");
    }
    // ---- the contig ids ----
    std::vector<uint32_t> h_cid;
    std::string names;
    int32_t C = 0;
    VSG(head, sizeof(int64_t) * (size_t)(n_runs + 1));
    VSG(run_cid, sizeof(uint32_t) * (size_t)(n_runs + 1));
    if (n_runs > 0) {
        hipLaunchKernelGGL(k_vs_heads, dim3(blocks_for(L)), dim3(VS_TPB), 0, st, P<int64_t>(ls), L, P<uint32_t>(flag),
                           P<uint32_t>(rid), n_runs, P<int64_t>(head));
        std::vector<int64_t> h_head((size_t)n_runs);
        VSK(hipMemcpyAsync(h_head.data(), head.p, sizeof(int64_t) * (size_t)n_runs, hipMemcpyDeviceToHost, st));
        VSK(hipStreamSynchronize(st));
        for (int64_t v : h_head)
            if (v < 0 || v >= n) return fail(GROM_E_HIP, "VCF sort: a run's head lies outside the stream");
        C = vs_map_names(chunks.data(), chunk, h_head.data(), n_runs, h_cid, names);
        VSK(hipMemcpyAsync(run_cid.p, h_cid.data(), sizeof(uint32_t) * (size_t)n_runs, hipMemcpyHostToDevice, st));
    }
    VSK(hipEventRecord(ev[1], st));
    // ---- sort ----
    for (VBuf *b : {&key, &key2}) VSG(*b, sizeof(uint64_t) * (size_t)(R + 1));
    for (VBuf *b : {&idx, &idx2}) VSG(*b, sizeof(uint32_t) * (size_t)(R + 1));
    for (VBuf *b : {&len, &doff}) VSG(*b, sizeof(int64_t) * (size_t)(R + 2));
    VSG(sorted, (size_t)n + 64);
    uint64_t *ks = P<uint64_t>(key), *ks2 = P<uint64_t>(key2);
    uint32_t *perm = P<uint32_t>(idx), *perm2 = P<uint32_t>(idx2);
    int np = 0;
    if (R > 0) {
        hipLaunchKernelGGL(k_vs_keys, dim3(blocks_for(R)), dim3(VS_TPB), 0, st, H, R, P<uint32_t>(rid), P<uint32_t>(run_cid),
                           n_runs, P<uint32_t>(pos), ks, perm, P<VsStat>(stat));
        VSK(hipMemcpyAsync(&hs, stat.p, sizeof(hs), hipMemcpyDeviceToHost, st));
        VSK(hipStreamSynchronize(st));
        int digit[8];
        np = vs_passes(hs.diff, digit);
        // one stable sort per stretch of adjacent digits that vary, the lowest first
        size_t tb_max = 0;
        for (int pass = 0; pass < 2; pass++) {
            if (pass == 1 && tmp.cap < tb_max) VSG(tmp, tb_max);
            for (int k = 0; k < np;) {
                int k1 = k;
                while (k1 + 1 < np && digit[k1 + 1] == digit[k1] + 1) k1++;
                size_t tb = tb_max;
                VSK(hipcub::DeviceRadixSort::SortPairs(pass ? tmp.p : nullptr, tb, ks, ks2, perm, perm2, (int)R, 8 * digit[k],
                                                       8 * digit[k1] + 8, st));
                if (pass) {
                    std::swap(ks, ks2);
                    std::swap(perm, perm2);
                } else {
                    tb_max = std::max(tb_max, tb);
                }
                k = k1 + 1;
            }
        }
    }
    // ---- gather ----
    int64_t h_hb = -1;  // the header's bytes: ls[H]
    VSK(hipMemcpyAsync(&h_hb, P<int64_t>(ls) + H, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    hipLaunchKernelGGL(k_vs_len, dim3(blocks_for(R + 1)), dim3(VS_TPB), 0, st, P<int64_t>(ls), H, R, perm, P<int64_t>(len));
    {
        size_t tb = 0;
        VSK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, P<int64_t>(len), P<int64_t>(doff), (int)(R + 1), st));
        if (tmp.cap < tb) {
            VSK(hipStreamSynchronize(st));
            VSG(tmp, tb);
        }
        VSK(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, P<int64_t>(len), P<int64_t>(doff), (int)(R + 1), st));
    }
    VSK(hipStreamSynchronize(st));
    if (h_hb < 0 || h_hb > n) return fail(GROM_E_HIP, "VCF sort: the header's end lies outside the stream");
    if (h_hb) VSK(hipMemcpyAsync(sorted.p, text.p, (size_t)h_hb, hipMemcpyDeviceToDevice, st));
    if (R > 0)
        hipLaunchKernelGGL(k_vs_gather, dim3(blocks_for(R * VS_SUB)), dim3(VS_TPB), 0, st, P<uint8_t>(text), n, P<int64_t>(ls), H, R,
                           perm, P<int64_t>(doff), h_hb, P<uint8_t>(sorted), n);
    VSK(hipGetLastError());
    VSK(hipEventRecord(ev[2], st));
    int64_t h_total = 0;
    VSK(hipMemcpyAsync(&h_total, P<int64_t>(doff) + R, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    for (int64_t o = 0; o < n; o += chunk)
        VSK(hipMemcpyAsync(chunks[(size_t)(o / chunk)], P<uint8_t>(sorted) + o, (size_t)std::min(chunk, n - o),
                           hipMemcpyDeviceToHost, st));
    VSK(hipStreamSynchronize(st));
    if (h_hb + h_total != n) return fail(GROM_E_HIP, "VCF sort: the sorted rows do not add up to the stream");
    // ---- the BGZF file, through the writer ----
    const std::string tag = ".tmp." + std::to_string((long long)getpid());
    const std::string tmp_gz = path + ".vs" + tag, tmp_tbi = path + ".tbi" + tag, tmp_gzi = path + ".gzi.vs" + tag;
    const int64_t n_blk = (n + VS_PAYLOAD - 1) / VS_PAYLOAD;
    std::vector<int64_t> h_coff((size_t)n_blk + 1);
    grom_bgzf_writer *bw = grom_bgzf_writer_open(tmp_gz.c_str(), device, tmp_gzi.c_str());
    if (!bw) return fail(GROM_E_HIP, grom_last_error());
    for (int64_t o = 0; o < n && rc == 0; o += chunk)
        rc = grom_bgzf_writer_write(bw, chunks[(size_t)(o / chunk)], std::min(chunk, n - o));
    if (rc == 0 && grom_bgzf_writer_block_offsets(bw, h_coff.data(), n_blk + 1) != n_blk) rc = GROM_E_HIP;
    const int rc2 = grom_bgzf_writer_close(bw, nullptr);
    if (rc || rc2) {
        fail(rc ? rc : rc2, grom_last_error());
        vs_commit(path, tmp_gz, tmp_tbi, tmp_gzi, false, err, sizeof(err));
        return failed;
    }
    // ---- index ----
    int64_t counts[3] = {0, 0, 0};
    std::vector<VsRun> h_runs;
    std::vector<VsSpan> h_span((size_t)C + 1);
    std::vector<int64_t> h_lb((size_t)C + 2, 0);
    std::vector<uint64_t> h_lin(1, VS_NONE);
    VSK(hipEventRecord(ev[3], st));
    VSK(hipEventRecord(ev[4], st));
    if (R > 0) {
        VSG(coff, sizeof(int64_t) * (size_t)(n_blk + 1));
        for (VBuf *b : {&vbeg, &vend}) VSG(*b, sizeof(uint64_t) * (size_t)(R + 1));
        for (VBuf *b : {&bin, &hf, &rinc}) VSG(*b, sizeof(uint32_t) * (size_t)(R + 1));
        VSG(maxw, sizeof(int32_t) * (size_t)(C + 1));
        VSG(span, sizeof(VsDevSpan) * (size_t)(C + 1));
        VSG(lin_base, sizeof(int64_t) * (size_t)(C + 2));
        VSK(hipMemcpyAsync(coff.p, h_coff.data(), sizeof(int64_t) * (size_t)(n_blk + 1), hipMemcpyHostToDevice, st));
        VSK(hipEventRecord(ev[3], st));
        VSK(hipMemsetAsync(maxw.p, 0, sizeof(int32_t) * (size_t)(C + 1), st));
        VSK(hipMemsetAsync(span.p, 0, sizeof(VsDevSpan) * (size_t)(C + 1), st));
        hipLaunchKernelGGL(k_vs_index, dim3(blocks_for(R)), dim3(VS_TPB), 0, st, H, R, L, perm, ks, P<int32_t>(beg), P<int32_t>(end),
                           P<int64_t>(doff), h_hb, P<int64_t>(coff), n_blk, n, C, P<uint64_t>(vbeg), P<uint64_t>(vend),
                           P<uint32_t>(bin), P<uint32_t>(hf), P<int32_t>(maxw), P<VsDevSpan>(span));
        if ((rc = scan_u32(P<uint32_t>(hf), P<uint32_t>(rinc), R, true)) != 0) return rc;
        uint32_t nr = 0;
        std::vector<int32_t> h_maxw((size_t)C);
        std::vector<VsDevSpan> d_span((size_t)C);
        VSK(hipMemcpyAsync(&nr, P<uint32_t>(rinc) + (R - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        VSK(hipMemcpyAsync(h_maxw.data(), maxw.p, sizeof(int32_t) * (size_t)C, hipMemcpyDeviceToHost, st));
        VSK(hipMemcpyAsync(d_span.data(), span.p, sizeof(VsDevSpan) * (size_t)C, hipMemcpyDeviceToHost, st));
        VSK(hipStreamSynchronize(st));
        for (int32_t c = 0; c < C; c++) {
            if (h_maxw[(size_t)c] < 0 || h_maxw[(size_t)c] > (int32_t)(VS_MAX_END >> 14)) return fail(GROM_E_HIP, "VCF sort: a contig's windows");
            h_lb[(size_t)c + 1] = h_lb[(size_t)c] + h_maxw[(size_t)c];
            h_span[(size_t)c] = VsSpan{d_span[(size_t)c].beg, d_span[(size_t)c].end,
                                      (uint64_t)(d_span[(size_t)c].j1 - d_span[(size_t)c].j0 + 1)};
        }
        const int64_t n_lin = h_lb[(size_t)C], n_ir = (int64_t)nr;
        VSG(runs, sizeof(VsRun) * (size_t)(n_ir + 1));
        VSG(lin, sizeof(uint64_t) * (size_t)(n_lin + 1));
        VSK(hipMemcpyAsync(lin_base.p, h_lb.data(), sizeof(int64_t) * (size_t)(C + 1), hipMemcpyHostToDevice, st));
        VSK(hipMemsetAsync(lin.p, 0xff, sizeof(uint64_t) * (size_t)(n_lin + 1), st));
        hipLaunchKernelGGL(k_vs_runs, dim3(blocks_for(R)), dim3(VS_TPB), 0, st, R, ks, P<uint32_t>(bin), P<uint64_t>(vbeg),
                           P<uint64_t>(vend), P<uint32_t>(hf), P<uint32_t>(rinc), P<VsRun>(runs), n_ir);
        hipLaunchKernelGGL(k_vs_linear, dim3(blocks_for(R)), dim3(VS_TPB), 0, st, H, R, L, perm, ks, P<int32_t>(beg), P<int32_t>(end),
                           P<uint64_t>(vbeg), P<int64_t>(lin_base), C, (unsigned long long *)lin.p);
        VSK(hipGetLastError());
        VSK(hipEventRecord(ev[4], st));
        h_runs.resize((size_t)n_ir);
        h_lin.assign((size_t)n_lin + 1, VS_NONE);
        if (n_ir) VSK(hipMemcpyAsync(h_runs.data(), runs.p, sizeof(VsRun) * (size_t)n_ir, hipMemcpyDeviceToHost, st));
        if (n_lin) VSK(hipMemcpyAsync(h_lin.data(), lin.p, sizeof(uint64_t) * (size_t)n_lin, hipMemcpyDeviceToHost, st));
        VSK(hipStreamSynchronize(st));
    } else {
        VSK(hipStreamSynchronize(st));
    }
    const bool ok = vs_write_tbi(tmp_tbi.c_str(), names, C, h_runs.data(), (int64_t)h_runs.size(), h_lin.data(), h_lb.data(),
                                 h_span.data(), counts, err, sizeof(err)) == 0;
    if (vs_commit(path, tmp_gz, tmp_tbi, tmp_gzi, ok, err, sizeof(err)) != 0) return fail(GROM_E_ARG, err);
    out[VS_O_ROWS] = R;
    out[VS_O_HEADER] = H;
    out[VS_O_CONTIGS] = C;
    out[VS_O_INVERSIONS] = (int64_t)hs.inv;
    out[VS_O_PASSES] = np;
    out[VS_O_BINS] = counts[0];
    out[VS_O_CHUNKS] = counts[1];
    out[VS_O_WINDOWS] = counts[2];
    out[VS_O_US_LINES] = (int64_t)(ms(0, 1) * 1000.0f) + 1;
    out[VS_O_US_SORT] = (int64_t)(ms(1, 2) * 1000.0f) + 1;
    out[VS_O_US_INDEX] = (int64_t)(ms(3, 4) * 1000.0f) + 1;
    return 0;
}

extern "C" grom_vcf_writer *grom_vcf_writer_open(const char *path, int device) {
    if (!path || !*path) {
        grom_set_last_error("VCF sort: no path");
        return nullptr;
    }
    grom_vcf_writer *w = new grom_vcf_writer;
    w->path = path;
    w->device = device < 0 ? -1 : device;
    w->chunk = chunk_bytes();
    if (w->device >= 0) {
        int ndev = 0;
        char m[256];
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || w->device >= ndev) {
            snprintf(m, sizeof(m), "VCF sort: no device %d (%d visible)", device, ndev);
            grom_set_last_error(m);
            w->device = -1;
            delete w;
            return nullptr;
        }
        DevGuard g(w->device);
        bool ok = g.ok && hipStreamCreateWithFlags(&w->st, hipStreamNonBlocking) == hipSuccess;
        for (hipEvent_t &e : w->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
        if (!ok) {
            snprintf(m, sizeof(m), "VCF sort: device %d cannot be used", device);
            grom_set_last_error(m);
            w->free_all();
            delete w;
            return nullptr;
        }
    }
    return w;
}

extern "C" int grom_vcf_writer_write(grom_vcf_writer *w, const void *buf, int64_t n) {
    if (!w || n < 0 || (n > 0 && !buf)) {
        grom_set_last_error("VCF sort: bad arguments");
        return GROM_E_ARG;
    }
    const uint8_t *p = (const uint8_t *)buf;
    while (n > 0 && !w->failed) {
        int64_t room = 0;
        uint8_t *dst = w->room(&room);
        if (!dst) break;
        const int64_t k = std::min<int64_t>(n, room);
        memcpy(dst, p, (size_t)k);
        w->n += k;
        p += k;
        n -= k;
    }
    if (w->failed) grom_set_last_error(w->err);
    return w->failed;
}

extern "C" int grom_vcf_writer_close(grom_vcf_writer *w, int64_t out[12]) {
    if (!w) return GROM_E_ARG;
    int64_t o[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!w->failed) {
        if (w->device < 0) {
            const std::vector<uint8_t> all = w->contiguous();
            const int rc = vs_host_run(all.data(), w->n, w->path.c_str(), o, w->err, sizeof(w->err));
            if (rc) w->fail(rc, w->err);
        } else {
            const int rc = w->run_device(o);
            if (rc) w->fail(rc, w->err);
        }
    }
    if (w->failed) grom_set_last_error(w->err);
    o[VS_O_US_WALL] = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - w->t0).count();
    if (out) memcpy(out, o, sizeof(o));
    const int rc = w->failed;
    w->free_all();
    delete w;
    return rc;
}

extern "C" int grom_vcf_tabix(const char *src, const char *dst, int device, int64_t out[12]) {
    if (out) memset(out, 0, 12 * sizeof(int64_t));
    char m[4600];
    FILE *fp = src ? fopen(src, "rb") : nullptr;
    if (!fp || !dst) {
        snprintf(m, sizeof(m), "VCF sort: cannot open %s", src ? src : "(no path)");
        grom_set_last_error(m);
        if (fp) fclose(fp);
        return GROM_E_ARG;
    }
    grom_vcf_writer *w = grom_vcf_writer_open(dst, device);
    if (!w) {
        fclose(fp);
        return device >= 0 ? GROM_E_NODEV : GROM_E_ARG;
    }
    for (;;) {  // read straight into the (pinned) chunks
        int64_t room = 0;
        uint8_t *dst = w->room(&room);
        if (!dst) break;
        const size_t got = fread(dst, 1, (size_t)room, fp);
        if (got == 0) break;
        w->n += (int64_t)got;
    }
    if (ferror(fp)) w->fail(GROM_E_ARG, "VCF sort: read error");
    fclose(fp);
    return grom_vcf_writer_close(w, out);
}
