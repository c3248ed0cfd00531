// baidev.hip -- a missing BAM index built on the device.
//
// The host builder (bai_build, bamio.c) inflates and walks every record of the
// file on one thread.  Here the file is read once (DdBgzfFile, ddecode.h: whole
// blocks through two pinned ring buffers) and goes through the device in
// pieces of whole BGZF blocks: the blocks are inflated by the decoder's
// inflater (dd_inflate_launch, ddecode.h) from the decoder's compressed
// slots (dd_comp_*), an index-free walk finds the record starts, one lane per
// record takes the facts an index needs (target id, begin, end, bin, the
// record's virtual offsets) and reductions turn them into the runs of records
// with one bin, the linear index and the counts.  The host joins the runs that
// continue across pieces and feeds them through bamio.c's merge rule and
// writer (bai_racc_add_run, bai_write_racc): the file is byte-identical to
// the host builder's.
//
// The walk has no index to start from, so it guesses and verifies on two
// levels.  The piece is cut at fixed offsets into chunks of IX_G bytes, IX_T
// chunks to a group (one workgroup).  Level 1: every lane guesses the first
// record start in its chunk (a header whose fields fit any target id in
// [-1, n_ref) and whose successor fits too) and walks to the chunk's end; lane
// 0 then follows the chain through the group from the group's first guess,
// taking a chunk's walk when its guess is where the chain enters it and
// walking the chunk again otherwise.  Level 2: one workgroup follows the
// chain through the groups from the piece's true start (the end of the header,
// or the first byte of the record carried over from the piece before): a
// group is taken when its first guess is the exit of the group before it,
// else it is walked again from the true position.  By induction every walk
// taken is the true chain's: a wrong guess costs time and never changes the
// result.  Candidates are arbitrary bytes: every load is bounded by the
// piece's length, and a chain that leaves the record limits is reported.
//
// The builder's device buffers are DevBufs (devbuf.h) accounted as decode
// memory: they grow to the largest piece and free themselves with the builder.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <unistd.h>

#include <hipcub/hipcub.hpp>

#include "../../include/grom_amd.h"
#include "bamio.h"
#include "ddecode.h"
#include "devbuf.h"

namespace {

#define IX_G 4096   // bytes per chunk (one lane)
#define IX_T 256    // chunks per group (one workgroup)
#define IX_MAX_REC (256 << 20)
#define IX_LIN_SLACK 64  // linear-index windows kept past a reference's end

enum : uint32_t { IXB_RECORD = 1, IXB_UNSORTED = 2, IXB_TID = 4, IXB_LINCAP = 8, IXB_VOFF = 16 };

// the misc words on the device: 32-bit [0] bad bits, [1] blocks that did not
// inflate, [2] block-table bounds, [3] chunks walked again; 64-bit (from byte
// 32) [0] the chain's exit of the piece, [1] unplaced records; 32-bit (from
// byte 64) the last record of the piece before, two copies of {valid, tid, pos, -};
// 32-bit (from byte 96) [0] blocks whose CRC-32 differs, [1] the lowest of them
// in the piece (the check of GROM_VERIFY_CRC / grom_bgzf_verify)
#define IX_MISC_BYTES 128
#define IX_CRC_WORD 24

// an unaligned word from two aligned ones (the caller checked p + 4 <= len; U
// is readable for 64 bytes past len)
__device__ __forceinline__ uint32_t ix_ld32(const uint8_t *U, int64_t p) {
    const uint32_t *a = (const uint32_t *)(U + (p & ~(int64_t)3));
    const uint32_t sh = (uint32_t)(p & 3) * 8;
    const uint32_t w0 = a[0];
    if (!sh) return w0;
    return (w0 >> sh) | (a[1] << (32 - sh));
}

__device__ __forceinline__ bool ix_fit(int32_t bs, int32_t tid, int32_t n_ref) {
    return bs >= 34 && bs <= (1 << 20) && tid >= -1 && tid < n_ref;
}

// could a record start at p?  (a guess: the chain decides)
__device__ bool ix_plausible(const uint8_t *U, int64_t p, int64_t len, int32_t n_ref) {
    if (p + 36 > len) return false;
    const int32_t bs = (int32_t)ix_ld32(U, p);
    if (!ix_fit(bs, (int32_t)ix_ld32(U, p + 4), n_ref)) return false;
    if ((int32_t)ix_ld32(U, p + 8) < -1) return false;
    const int lqn = (int)(ix_ld32(U, p + 12) & 0xff), nc = (int)(ix_ld32(U, p + 16) & 0xffff);
    const int32_t lq = (int32_t)ix_ld32(U, p + 20), mtid = (int32_t)ix_ld32(U, p + 24);
    if (lqn < 1 || lq < 0 || 32 + (int64_t)lqn + 4 * (int64_t)nc + (lq + 1) / 2 + lq > (int64_t)bs) return false;
    if (mtid < -1 || mtid >= n_ref || (int32_t)ix_ld32(U, p + 28) < -1) return false;
    if (p + 36 + lqn > len || U[p + 36 + lqn - 1] != 0) return false;
    const int64_t q = p + 4 + (int64_t)bs;
    if (q + 8 <= len && !ix_fit((int32_t)ix_ld32(U, q), (int32_t)ix_ld32(U, q + 4), n_ref)) return false;
    return true;
}

// the first plausible record start in [lo, hi), -1 none: block_size and the
// target id of every position from a sliding window of three aligned words
__device__ int64_t ix_guess(const uint8_t *U, int64_t lo, int64_t hi, int64_t len, int32_t n_ref) {
    int64_t a = lo & ~(int64_t)3;
    const uint32_t *wp = (const uint32_t *)(U + a);
    uint32_t w0 = wp[0], w1 = wp[1], w2 = wp[2];
    for (int64_t i = 3; a < hi; a += 4, i++) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t p = a + k;
            const uint32_t bs = k ? (w0 >> (8 * k)) | (w1 << (32 - 8 * k)) : w0;
            const uint32_t td = k ? (w1 >> (8 * k)) | (w2 << (32 - 8 * k)) : w1;
            if (p >= lo && p < hi && ix_fit((int32_t)bs, (int32_t)td, n_ref) && ix_plausible(U, p, len, n_ref)) return p;
        }
        w0 = w1;
        w1 = w2;
        w2 = wp[i];  // (at most 16 bytes past hi <= len: inside U's slack)
    }
    return -1;
}

// records from o while they start below hi and end inside the piece: their
// number, (off != nullptr) their offsets, and the exit.  An exit below hi: the
// record there does not end in the piece (it is carried to the next one); -1:
// a block_size outside the record limits
__device__ int64_t ix_walk(const uint8_t *U, int64_t o, int64_t hi, int64_t len, uint32_t &n, int64_t *off,
                           uint32_t off_cap) {
    n = 0;
    while (o < hi) {
        if (o + 4 > len) break;
        const int32_t bs = (int32_t)ix_ld32(U, o);
        if (bs < 32 || bs > IX_MAX_REC) return -1;
        if (o + 4 + (int64_t)bs > len) break;
        if (off && n < off_cap) off[n] = o;
        o += 4 + (int64_t)bs;
        n++;
    }
    return o;
}

struct IxShared {
    int64_t start[IX_T], exit[IX_T];
    uint32_t n[IX_T];
    int64_t carry, entry;
    int fail;
};

// One group: the chunks q0 .. q0 + m - 1 (chunk q is [base + q IX_G, + IX_G),
// cut at len).  known >= 0: where the true chain enters the group; else the
// group's first guess stands in for it (sh.entry, -1: no guess in the group).
// Every chunk's chain start and record count go to sub_st / sub_n, the chain's
// exit to sh.carry; sh.fail: the chain left the record limits.  guess: 1
// plausible headers, 0 none, 2 the chunks' own first bytes (mostly wrong: tests)
__device__ void ix_group(const uint8_t *U, int64_t len, int64_t base, int64_t q0, int m, int64_t known, int guess,
                         int32_t n_ref, IxShared &sh, int64_t *sub_st, uint32_t *sub_n, uint32_t *rewalk) {
    const int t = threadIdx.x;
    int64_t st = -1, ex = -1;
    uint32_t n = 0;
    if (t < m && !(known >= 0 && t == 0)) {
        const int64_t lo = base + (q0 + t) * IX_G, hi = lo + IX_G < len ? lo + IX_G : len;
        if (guess == 2) st = lo;
        else if (guess == 1) st = ix_guess(U, lo, hi, len, n_ref);
        if (st >= 0) ex = ix_walk(U, st, hi, len, n, nullptr, 0);
    }
    sh.start[t] = st;
    sh.exit[t] = ex;
    sh.n[t] = n;
    __syncthreads();
    if (t == 0) {
        int64_t carry = known;
        for (int k = 0; k < m && carry < 0; k++) carry = sh.start[k];
        sh.entry = carry;
        int fail = 0;
        uint32_t again = 0;
        for (int k = 0; k < m && carry >= 0; k++) {
            const int64_t lo = base + (q0 + k) * IX_G, khi = lo + IX_G < len ? lo + IX_G : len;
            if (carry >= khi) {  // a record spans the chunk: no start in it
                sh.start[k] = carry;
                sh.n[k] = 0;
                continue;
            }
            if (sh.start[k] == carry && sh.exit[k] >= 0) {
                carry = sh.exit[k];
                continue;
            }
            if (sh.start[k] >= 0) again++;
            uint32_t kn = 0;
            const int64_t kex = ix_walk(U, carry, khi, len, kn, nullptr, 0);
            if (kex < 0) { fail = 1; break; }
            sh.start[k] = carry;
            sh.n[k] = kn;
            carry = kex;
        }
        if (again) atomicAdd(rewalk, again);
        sh.carry = carry;
        sh.fail = fail;
    }
    __syncthreads();
    if (t < m) {
        const bool ok = !sh.fail && sh.entry >= 0;
        sub_st[q0 + t] = ok ? sh.start[t] : -1;
        sub_n[q0 + t] = ok ? sh.n[t] : 0u;
    }
    __syncthreads();
}

// level 1: one workgroup per group; group 0 starts at the piece's true start
__global__ void __launch_bounds__(IX_T) k_ix_sub(const uint8_t *__restrict__ U, int64_t len, int64_t base, int64_t nsub,
                                                 int guess, int32_t n_ref, int64_t *__restrict__ sub_st,
                                                 uint32_t *__restrict__ sub_n, int64_t *__restrict__ cg,
                                                 int64_t *__restrict__ cex, uint32_t *__restrict__ m32) {
    __shared__ IxShared sh;
    const int64_t c = blockIdx.x, q0 = c * IX_T;
    if (q0 >= nsub) return;
    const int m = (int)(nsub - q0 < IX_T ? nsub - q0 : IX_T);
    ix_group(U, len, base, q0, m, c == 0 ? base : -1, guess, n_ref, sh, sub_st, sub_n, m32 + 3);
    if (threadIdx.x == 0) {
        const bool ok = !sh.fail && sh.entry >= 0;
        cg[c] = ok ? sh.entry : -1;
        cex[c] = ok ? sh.carry : -1;
    }
}

// level 2: one workgroup follows the chain through the groups
__global__ void __launch_bounds__(IX_T) k_ix_chain(const uint8_t *__restrict__ U, int64_t len, int64_t base,
                                                   int64_t nsub, int64_t nch, int guess, int32_t n_ref,
                                                   int64_t *__restrict__ sub_st, uint32_t *__restrict__ sub_n,
                                                   const int64_t *__restrict__ cg, const int64_t *__restrict__ cex,
                                                   uint32_t *__restrict__ m32, int64_t *__restrict__ m64) {
    __shared__ IxShared sh;
    __shared__ int64_t s_cg[IX_T], s_cex[IX_T];
    __shared__ int64_t s_c;
    __shared__ int s_k;
    const int t = threadIdx.x;
    if (t == 0) s_c = cex[0];
    __syncthreads();
    if (s_c < 0) {  // the true chain left the record limits in group 0
        if (t == 0) { atomicOr(m32, (uint32_t)IXB_RECORD); m64[0] = -1; }
        return;
    }
    for (int64_t b0 = 1; b0 < nch; b0 += IX_T) {
        const int mb = (int)(nch - b0 < IX_T ? nch - b0 : IX_T);
        if (t < mb) { s_cg[t] = cg[b0 + t]; s_cex[t] = cex[b0 + t]; }
        if (t == 0) s_k = 0;
        __syncthreads();
        for (;;) {
            if (t == 0) {
                int k = s_k;
                int64_t carry = s_c;
                while (k < mb && s_cg[k] == carry && s_cex[k] >= 0) { carry = s_cex[k]; k++; }
                s_k = k;
                s_c = carry;
            }
            __syncthreads();
            const int k = s_k;
            const int64_t known = s_c;
            __syncthreads();
            if (k >= mb) break;
            const int64_t q0 = (b0 + k) * IX_T;
            const int m = (int)(nsub - q0 < IX_T ? nsub - q0 : IX_T);
            ix_group(U, len, base, q0, m, known, guess, n_ref, sh, sub_st, sub_n, m32 + 3);
            if (sh.fail) {
                if (t == 0) { atomicOr(m32, (uint32_t)IXB_RECORD); m64[0] = -1; }
                return;
            }
            if (t == 0) { s_c = sh.carry; s_k = k + 1; }
            __syncthreads();
        }
    }
    if (t == 0) m64[0] = s_c;
}

// every record's offset: one lane per chunk, from the chunk's verified start
__global__ void k_ix_offsets(const uint8_t *__restrict__ U, int64_t len, int64_t base, int64_t nsub,
                             const int64_t *__restrict__ sub_st, const uint32_t *__restrict__ sub_n,
                             const uint32_t *__restrict__ sub_base, int64_t *__restrict__ off, int64_t R,
                             uint32_t *__restrict__ m32) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nsub) return;
    const uint32_t n = sub_n[q];
    if (n == 0) return;
    const int64_t st = sub_st[q], w = sub_base[q], lo = base + q * IX_G, hi = lo + IX_G < len ? lo + IX_G : len;
    if (st < 0 || w + (int64_t)n > R) { atomicOr(m32, (uint32_t)IXB_RECORD); return; }
    uint32_t n2 = 0;
    ix_walk(U, st, hi, len, n2, off + w, n);
    if (n2 != n) atomicOr(m32, (uint32_t)IXB_RECORD);
}

// the virtual offset of byte x of the piece, as bgzf_tell gives it: tu[i] is
// block i's first byte in the piece (the blocks under the carried bytes
// included, the last entry the block after the piece), tc[i] its file offset;
// a position at a block's end is the next block's start, an empty block too
__device__ __forceinline__ bool ix_voff(const int64_t *__restrict__ tu, const int64_t *__restrict__ tc, int nt, int64_t x,
                                        uint64_t &v) {
    int lo = 0, hi = nt;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tu[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    if (lo < nt && tu[lo] == x) { v = (uint64_t)tc[lo] << 16; return true; }
    if (lo == 0 || lo >= nt) return false;
    const int64_t d = x - tu[lo - 1];
    if (d <= 0 || d >= 65536) return false;
    v = ((uint64_t)tc[lo - 1] << 16) | (uint64_t)d;
    return true;
}

__device__ __forceinline__ int ix_reg2bin(int32_t beg, int32_t end) {
    --end;
    if (beg >> 14 == end >> 14) return ((1 << 15) - 1) / 7 + (beg >> 14);
    if (beg >> 17 == end >> 17) return ((1 << 12) - 1) / 7 + (beg >> 17);
    if (beg >> 20 == end >> 20) return ((1 << 9) - 1) / 7 + (beg >> 20);
    if (beg >> 23 == end >> 23) return ((1 << 6) - 1) / 7 + (beg >> 23);
    if (beg >> 26 == end >> 26) return ((1 << 3) - 1) / 7 + (beg >> 26);
    return 0;
}

// one lane per record: target id, position, end (bam_end_pos), bin (bit 31:
// flagged unmapped) and the record's begin and end virtual offsets
__global__ void k_ix_facts(const uint8_t *__restrict__ U, int64_t len, const int64_t *__restrict__ off, int64_t R,
                           const int64_t *__restrict__ tu, const int64_t *__restrict__ tc, int nt,
                           int32_t *__restrict__ tid, int32_t *__restrict__ pos, int32_t *__restrict__ end,
                           uint32_t *__restrict__ binu, uint64_t *__restrict__ vbeg, uint64_t *__restrict__ vend,
                           uint32_t *__restrict__ m32) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= R) return;
    const int64_t o = off[j];
    int32_t td = -1, ps = -1, en = 0;
    uint32_t bn = 0;
    uint64_t vb = 0, ve = 0;
    bool ok = o >= 0 && o + 36 <= len;
    int32_t bs = 0;
    if (ok) {
        bs = (int32_t)ix_ld32(U, o);
        ok = bs >= 32 && o + 4 + (int64_t)bs <= len;
    }
    if (ok) {
        td = (int32_t)ix_ld32(U, o + 4);
        ps = (int32_t)ix_ld32(U, o + 8);
        const int lqn = (int)(ix_ld32(U, o + 12) & 0xff);
        const uint32_t w4 = ix_ld32(U, o + 16);
        const int nc = (int)(w4 & 0xffff), flag = (int)(w4 >> 16);
        uint32_t rl = 0;
        if (!(flag & 4)) {
            if (32 + (int64_t)lqn + 4 * (int64_t)nc > (int64_t)bs) ok = false;
            for (int i = 0; ok && i < nc; i++) {
                const uint32_t c = ix_ld32(U, o + 36 + lqn + 4 * (int64_t)i);
                const uint32_t op = c & 15u;
                if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += c >> 4;
            }
        }
        en = (int32_t)((uint32_t)ps + ((int32_t)rl > 0 ? rl : 1u));
        bn = (uint32_t)ix_reg2bin(ps < 0 ? 0 : ps, en) | ((flag & 4) ? 0x80000000u : 0u);
        if (!ix_voff(tu, tc, nt, o, vb) || !ix_voff(tu, tc, nt, o + 4 + (int64_t)bs, ve)) atomicOr(m32, (uint32_t)IXB_VOFF);
    }
    if (!ok) atomicOr(m32, (uint32_t)IXB_RECORD);
    tid[j] = td;
    pos[j] = ps;
    end[j] = en;
    binu[j] = bn;
    vbeg[j] = vb;
    vend[j] = ve;
}

// one lane per record against the record before it (the piece's first: the
// last record of the piece before, st_in): the sortedness check, the run
// heads, the unplaced count and the linear index.  A record writes a window
// only when the record before it does not overlap that window: that one, or
// one before it, has the smaller offset.  key[j] = head << 32 | unmapped
__global__ void k_ix_reduce(int64_t R, const int32_t *__restrict__ tid, const int32_t *__restrict__ pos,
                            const int32_t *__restrict__ end, const uint32_t *__restrict__ binu,
                            const uint64_t *__restrict__ vbeg, int32_t n_ref,
                            unsigned long long *__restrict__ lin, const int64_t *__restrict__ lin_base,
                            uint64_t *__restrict__ key, uint32_t *__restrict__ m32,
                            unsigned long long *__restrict__ n_unplaced, const int32_t *__restrict__ st_in,
                            int32_t *__restrict__ st_out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= R) return;
    const int32_t t = tid[j], p = pos[j], e = end[j];
    const uint32_t b = binu[j];
    int pv, pt, pp, pe = 0;
    uint32_t pb = 0xffffffffu;
    if (j > 0) { pv = 1; pt = tid[j - 1]; pp = pos[j - 1]; pe = end[j - 1]; pb = binu[j - 1]; }
    else { pv = st_in[0]; pt = st_in[1]; pp = st_in[2]; }
    uint64_t k = 0;
    if (t < 0) {
        atomicAdd(n_unplaced, 1ull);
    } else if (t >= n_ref) {
        atomicOr(m32, (uint32_t)IXB_TID);
    } else {
        // a placed record after an unplaced one, or out of order (bamio.c, bai_build)
        if (pv && (pt < 0 || t < pt || (t == pt && p < pp))) atomicOr(m32, (uint32_t)IXB_UNSORTED);
        const bool head = j == 0 || pt != t || (pb & 0x7fffffffu) != (b & 0x7fffffffu);
        k = ((uint64_t)(head ? 1 : 0) << 32) | (b >> 31);
        const int32_t w0 = (p < 0 ? 0 : p) >> 14, w1 = (e - 1) >> 14;
        int32_t pw0 = 0, pw1 = -1;
        if (j > 0 && pt == t) { pw0 = (pp < 0 ? 0 : pp) >> 14; pw1 = (pe - 1) >> 14; }
        const int64_t lb = lin_base[t], cap = lin_base[t + 1] - lb;
        const unsigned long long vb = vbeg[j];
        for (int32_t w = w0; w <= w1; w++) {
            if (w >= pw0 && w <= pw1) continue;
            if (w >= cap) { atomicOr(m32, (uint32_t)IXB_LINCAP); break; }
            atomicMin(&lin[lb + w], vb);
        }
    }
    key[j] = k;
    if (j == R - 1) { st_out[0] = 1; st_out[1] = t; st_out[2] = p; }
}

// one run of records with one target id and bin: its first begin offset and
// last end offset; records j0..j1, u1 - u0 of them flagged unmapped
struct IxRun {
    int32_t tid;
    uint32_t bin;
    uint64_t beg, end;
    uint32_t j0, j1, u0, u1;
};

// pre = the exclusive sum of key: the run a record belongs to, the unmapped before it
__global__ void k_ix_runs(int64_t R, const int32_t *__restrict__ tid, const uint32_t *__restrict__ binu,
                          const uint64_t *__restrict__ vbeg, const uint64_t *__restrict__ vend,
                          const uint64_t *__restrict__ key, const uint64_t *__restrict__ pre,
                          IxRun *__restrict__ runs, int64_t n_runs, int32_t n_ref) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= R) return;
    const int32_t t = tid[j];
    if (t < 0 || t >= n_ref) return;
    const uint64_t k = key[j], pr = pre[j];
    const bool head = (k >> 32) != 0;
    const int64_t r = (int64_t)(pr >> 32) + (head ? 1 : 0) - 1;
    if (r < 0 || r >= n_runs) return;
    if (head) {
        runs[r].tid = t;
        runs[r].bin = binu[j] & 0x7fffffffu;
        runs[r].beg = vbeg[j];
        runs[r].j0 = (uint32_t)j;
        runs[r].u0 = (uint32_t)pr;
    }
    const bool last = j == R - 1 || (key[j + 1] >> 32) != 0 || tid[j + 1] < 0 || tid[j + 1] >= n_ref;
    if (last) {
        runs[r].end = vend[j];
        runs[r].j1 = (uint32_t)j;
        runs[r].u1 = (uint32_t)pr + (uint32_t)k;
    }
}

using Buf = DevBufOf<GROM_DEVCAT_DECODE, 256>;  // decode memory, an eighth of slack (devbuf.h)

// the BAM header through the host reader: its length in the inflated stream
// (the first record's position) and the references' lengths
int ix_read_header(const char *path, int64_t *hdr_len, std::vector<int32_t> &ref_len) {
    bgzf_reader r;
    if (bgzf_open_read(&r, path) != 0) return -1;
    int rc = -1;
    int64_t n = 0;
    unsigned char b4[4];
    std::vector<unsigned char> skip(65536);
    auto rd = [&](void *dst, int k) { if (k && bgzf_read(&r, dst, k) != k) return false; n += k; return true; };
    auto u32 = [&] { return (int32_t)((uint32_t)b4[0] | (uint32_t)b4[1] << 8 | (uint32_t)b4[2] << 16 | (uint32_t)b4[3] << 24); };
    auto skipn = [&](int64_t k) {
        while (k > 0) {
            const int s = (int)std::min<int64_t>(k, (int64_t)skip.size());
            if (!rd(skip.data(), s)) return false;
            k -= s;
        }
        return true;
    };
    do {
        if (!rd(b4, 4) || memcmp(b4, "BAM\1", 4) != 0) break;
        if (!rd(b4, 4) || u32() < 0 || !skipn(u32())) break;
        if (!rd(b4, 4)) break;
        const int32_t n_ref = u32();
        if (n_ref < 0) break;
        bool ok = true;
        for (int32_t i = 0; i < n_ref && ok; i++) {
            ok = rd(b4, 4) && u32() >= 0 && skipn(u32()) && rd(b4, 4);
            if (ok) ref_len.push_back(u32());
        }
        if (!ok) break;
        rc = 0;
    } while (0);
    bgzf_close_read(&r);
    *hdr_len = n;
    return rc;
}

struct HostBlk {
    int64_t abs_off, c_off;  // its first byte in the file's inflated stream; the block's file offset
    uint32_t len;
};

// one piece as read from the file (DdBgzfFile): whole blocks from file offset c0 on
struct PieceIn {
    std::vector<DdBlock> blk;  // in_off in the piece's compressed bytes, out_off from 0
    int64_t nblk = 0, comp_len = 0, ubytes = 0, c0 = 0;
    bool last = false;
};

struct IxBuild {
    int device = 0, guess = 1;
    bool verify = false;         // every piece's blocks against their CRC-32 (read once, in init)
    const char *path = nullptr;  // ... and a mismatch names the file
    double ms_crc = 0;
    hipEvent_t ev_crc = nullptr;
    int64_t piece_bytes = (int64_t)3 << 30, comp_read = (int64_t)256 << 20;
    DdBgzfFile in;  // the BAM, read in whole blocks through two pinned ring buffers
    std::vector<int32_t> ref_len;
    int32_t n_ref = 0;
    dd_ctx *ctx = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t ev[5] = {};
    int64_t *h_small = nullptr;  // pinned: the misc words (16 x 8 bytes), then two scalars
    PieceIn pin[2];
    Buf U[2], dblk, status, tok, misc, sub_st, sub_n, sub_base, cg, cex, tmp, tu, tc, off, tid, pos, end, binu, vbeg,
        vend, key, pre, runs, lin, lin_base;
    std::vector<HostBlk> keep;
    std::vector<int64_t> h_tu, h_tc, h_lin_base;
    std::vector<IxRun> h_runs;
    // assembly
    std::vector<bai_racc *> racc;
    std::vector<uint64_t> off_beg, off_end, n_map, n_unm;
    std::vector<char> any;
    bool pend = false;
    IxRun cur = {};
    int64_t n_rec = 0, n_blk = 0, n_piece = 0, n_sub = 0, n_runs = 0;
    double ms_inflate = 0, ms_walk = 0, ms_reduce = 0;
    char err[512] = {0};

    explicit IxBuild(const char *bam_path) : path(bam_path), in(bam_path) {}
    // the stream is drained and the decode context (whose copy stream reads
    // the ring buffers) freed here; the buffers and `in` free themselves after
    ~IxBuild() {
        if (st) (void)hipStreamSynchronize(st);
        if (ctx) dd_ctx_free(ctx);
        for (int k = 0; k < 5; k++)
            if (ev[k]) (void)hipEventDestroy(ev[k]);
        if (ev_crc) (void)hipEventDestroy(ev_crc);
        if (h_small) (void)hipHostFree(h_small);
        if (st) (void)hipStreamDestroy(st);
        for (bai_racc *a : racc) bai_racc_free(a);
    }

    int fail(int code, const char *fmt, long long a = 0, long long b = 0) {
        snprintf(err, sizeof(err), fmt, a, b);
        return code;
    }
#define IXK(x)                                                                                                    \
    do {                                                                                                          \
        hipError_t e_ = (x);                                                                                      \
        if (e_ != hipSuccess) {                                                                                   \
            snprintf(err, sizeof(err), "device index build: HIP error %s at %s:%d", hipGetErrorString(e_), __FILE__, \
                     __LINE__);                                                                                   \
            return GROM_E_HIP;                                                                                    \
        }                                                                                                         \
    } while (0)
#define IXG(b, bytes)                                                                                                 \
    do {                                                                                                              \
        if ((b).grow(bytes)) return fail(GROM_E_NOMEM, "device index build: hipMalloc(%lld) failed", (long long)(bytes)); \
    } while (0)

    // the next piece's blocks read into ring buffer s and sent to compressed slot s
    int read_piece(int s) {
        PieceIn &p = pin[s];
        p.nblk = 0;
        p.comp_len = p.ubytes = 0;
        p.c0 = in.off;
        p.last = false;
        p.blk.clear();
        if (in.off >= in.size) return 0;
        if (dd_comp_ring_wait(ctx, s) != 0) return fail(GROM_E_HIP, "device index build: the copy ring failed");
        const int64_t nb = in.read(s, piece_bytes, &p.comp_len, &p.ubytes);
        if (nb == DD_READ_IO) return fail(GROM_E_ARG, "device index build: read error at byte %lld", (long long)in.off);
        if (nb <= 0) return fail(GROM_E_ARG, "device index build: no whole BGZF block at byte %lld", (long long)in.off);
        p.blk.assign(in.tab.begin(), in.tab.begin() + nb);
        p.nblk = nb;
        p.last = in.off >= in.size;
        if (dd_comp_begin(ctx, s, p.comp_len, err, sizeof(err)) != 0 ||
            dd_comp_chunk(ctx, s, s, in.ring[s], 0, p.comp_len, err, sizeof(err)) != 0 ||
            dd_comp_end(ctx, s, p.comp_len, err, sizeof(err)) != 0)
            return GROM_E_HIP;
        return 0;
    }

    // a finished run of the device's list into the accumulators (runs of one
    // target id and bin that meet at a piece boundary are one run)
    void push_run(const IxRun &r) {
        const uint64_t n = (uint64_t)r.j1 - r.j0 + 1, unm = (uint64_t)r.u1 - r.u0;
        const size_t t = (size_t)r.tid;
        if (!any[t]) { any[t] = 1; off_beg[t] = r.beg; }
        off_end[t] = r.end;
        n_map[t] += n - unm;
        n_unm[t] += unm;
        if (pend && cur.tid == r.tid && cur.bin == r.bin) {
            cur.end = r.end;
            return;
        }
        flush_run();
        cur = r;
        pend = true;
    }
    void flush_run() {
        if (!pend) return;
        bai_racc_add_run(racc[(size_t)cur.tid], cur.bin, cur.beg, cur.end);
        n_runs++;
        pend = false;
    }

    int init() {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess)
            return fail(GROM_E_NODEV, "device index build: no device %lld (%lld visible)", device, ndev);
        const char *e = getenv("GROM_INDEX_PIECE_KB");
        if (e && atof(e) > 0) piece_bytes = std::max<int64_t>((int64_t)(atof(e) * 1024.0), 4096);
        if (getenv("GROM_INDEX_GUESS")) guess = atoi(getenv("GROM_INDEX_GUESS"));
        verify = bgzf_verify_on() != 0;
        comp_read = std::min<int64_t>(comp_read, std::max<int64_t>(piece_bytes, 65536) + 65536);
        comp_read = std::min<int64_t>(comp_read, in.size);
        comp_read = std::max<int64_t>(comp_read, 4096);
        ctx = dd_ctx_new(device);
        if (!ctx) return fail(GROM_E_HIP, "device index build: no decode context on device %lld", device);
        IXK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        for (int k = 0; k < 5; k++) IXK(hipEventCreate(&ev[k]));
        if (verify) IXK(hipEventCreate(&ev_crc));
        IXK((hipError_t)in.rings(comp_read, (size_t)(comp_read / 512 + 64)));
        IXK(hipHostMalloc((void **)&h_small, 32 * sizeof(int64_t), 0));
        IXG(misc, IX_MISC_BYTES);
        IXK(hipMemsetAsync(misc.p, 0, IX_MISC_BYTES, st));
        // the linear index of every reference: the windows of its length and some past it
        h_lin_base.assign((size_t)n_ref + 1, 0);
        for (int32_t t = 0; t < n_ref; t++)
            h_lin_base[(size_t)t + 1] = h_lin_base[(size_t)t] + ((int64_t)(ref_len[(size_t)t] > 0 ? ref_len[(size_t)t] : 0) >> 14) + 1 + IX_LIN_SLACK;
        IXG(lin_base, 8 * ((size_t)n_ref + 1));
        IXG(lin, 8 * (size_t)std::max<int64_t>(h_lin_base[(size_t)n_ref], 1));
        IXK(hipMemcpyAsync(lin_base.p, h_lin_base.data(), 8 * ((size_t)n_ref + 1), hipMemcpyHostToDevice, st));
        IXK(hipMemsetAsync(lin.p, 0xff, 8 * (size_t)std::max<int64_t>(h_lin_base[(size_t)n_ref], 1), st));
        IXK(hipStreamSynchronize(st));
        racc.assign((size_t)n_ref, nullptr);
        for (int32_t t = 0; t < n_ref; t++)
            if (!(racc[(size_t)t] = bai_racc_new())) return fail(GROM_E_NOMEM, "device index build: out of memory");
        off_beg.assign((size_t)n_ref, 0);
        off_end.assign((size_t)n_ref, 0);
        n_map.assign((size_t)n_ref, 0);
        n_unm.assign((size_t)n_ref, 0);
        any.assign((size_t)n_ref, 0);
        return 0;
    }

    int check_bad(const uint32_t *m32) {
        if (m32[1] || m32[2]) return fail(GROM_E_ARG, "device index build: %lld BGZF blocks did not inflate", m32[1]);
        if (m32[0] & IXB_RECORD) return fail(GROM_E_ARG, "device index build: a record's sizes are outside its limits");
        if (m32[0] & IXB_VOFF) return fail(GROM_E_ARG, "device index build: a record lies outside the piece's blocks");
        if (m32[0] & IXB_TID) return fail(GROM_E_ARG, "device index build: a target id is not below the header's %lld", n_ref);
        if (m32[0] & IXB_UNSORTED) return fail(GROM_E_ARG, "device index build: the BAM is not sorted by coordinate");
        if (m32[0] & IXB_LINCAP)
            return fail(GROM_E_ARG, "device index build: a record ends more than %lld windows past its reference's length",
                        IX_LIN_SLACK);
        return 0;
    }

    int run(int64_t hdr_len) {
        int rc = init();
        if (rc) return rc;
        int64_t origin = 0;     // the file's inflated offset of the next piece's first byte
        int64_t abs_end = 0;    // ... of the first block not yet taken
        int64_t carry_len = 0;  // bytes of the record carried into the next piece
        int64_t carry_pos = 0;  // where they lie in the piece before
        int64_t start = hdr_len;
        int n_state = 0;
        if ((rc = read_piece(0)) != 0) return rc;
        for (int64_t k = 0;; k++) {
            const int s = (int)(k & 1);
            PieceIn &p = pin[s];
            if (p.nblk == 0) {
                if (in.off < in.size) return fail(GROM_E_ARG, "device index build: no whole BGZF block at byte %lld", in.off);
                if (carry_len != 0 || start > 0) return fail(GROM_E_ARG, "device index build: the BAM ends inside a record");
                break;
            }
            n_piece++;
            n_blk += p.nblk;
            for (int64_t i = 0; i < p.nblk; i++) {
                keep.push_back({abs_end, p.c0 + p.blk[(size_t)i].c_off, p.blk[(size_t)i].out_len});
                abs_end += p.blk[(size_t)i].out_len;
            }
            const int64_t ulen = carry_len + p.ubytes;
            if (carry_len == 0 && start >= ulen) {  // still inside the header
                start -= ulen;
                origin += ulen;
                if ((rc = read_piece(s ^ 1)) != 0) return rc;
                if (p.last) {
                    if (start > 0) return fail(GROM_E_ARG, "device index build: the BAM ends inside its header");
                    break;
                }
                continue;
            }
            // ---- phase A: inflate, the two-level walk, the chunks' record counts ----
            IXG(U[s], (size_t)ulen + 64);
            uint8_t *Up = P<uint8_t>(U[s]);
            if (carry_len) IXK(hipMemcpyAsync(Up, P<uint8_t>(U[s ^ 1]) + carry_pos, (size_t)carry_len, hipMemcpyDeviceToDevice, st));
            IXK(hipMemsetAsync(Up + ulen, 0, 64, st));
            for (int64_t i = 0, o = carry_len; i < p.nblk; i++) {
                p.blk[(size_t)i].out_off = o;
                o += p.blk[(size_t)i].out_len;
            }
            IXG(dblk, sizeof(DdBlock) * (size_t)(p.nblk + 1));
            IXG(status, (size_t)p.nblk + 16);
            const size_t tokb = dd_inflate_tok_bytes(p.nblk);
            if (tokb) IXG(tok, tokb);
            IXK(hipMemcpyAsync(dblk.p, p.blk.data(), sizeof(DdBlock) * (size_t)p.nblk, hipMemcpyHostToDevice, st));
            // the blocks under the piece's bytes, and the block after it
            h_tu.clear();
            h_tc.clear();
            for (const HostBlk &b : keep) { h_tu.push_back(b.abs_off - origin); h_tc.push_back(b.c_off); }
            h_tu.push_back(abs_end - origin);
            h_tc.push_back(foff_after(p));
            const int nt = (int)h_tu.size();
            IXG(tu, 8 * (size_t)nt);
            IXG(tc, 8 * (size_t)nt);
            IXK(hipMemcpyAsync(tu.p, h_tu.data(), 8 * (size_t)nt, hipMemcpyHostToDevice, st));
            IXK(hipMemcpyAsync(tc.p, h_tc.data(), 8 * (size_t)nt, hipMemcpyHostToDevice, st));
            const int64_t nsub = (ulen - start + IX_G - 1) / IX_G, nch = (nsub + IX_T - 1) / IX_T;
            n_sub += nsub;
            IXG(sub_st, 8 * (size_t)(nsub + 1));
            IXG(sub_n, 4 * (size_t)(nsub + 1));
            IXG(sub_base, 4 * (size_t)(nsub + 1));
            IXG(cg, 8 * (size_t)nch);
            IXG(cex, 8 * (size_t)nch);
            size_t tb = 0;
            IXK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (uint32_t *)nullptr, (uint32_t *)nullptr, (int)(nsub + 1), st));
            IXG(tmp, tb);
            const uint8_t *d_comp = nullptr;
            int64_t comp_cap = 0;
            if (dd_comp_view(ctx, s, &d_comp, &comp_cap) != 0 || comp_cap < p.comp_len || dd_comp_wait_on(ctx, s, (void *)st) != 0)
                return fail(GROM_E_HIP, "device index build: compressed slot %lld is not filled", s);
            uint32_t *m32 = P<uint32_t>(misc);
            int64_t *m64 = (int64_t *)(P<uint8_t>(misc) + 32);
            int32_t *dstate = (int32_t *)(P<uint8_t>(misc) + 64);
            IXK(hipEventRecord(ev[0], st));
            if (dd_inflate_launch(st, d_comp, p.comp_len, P<DdBlock>(dblk), p.nblk, Up, 0, ulen, P<uint8_t>(status), m32 + 1,
                                  m32 + 2, tokb ? P<uint32_t>(tok) : nullptr, tokb ? tok.cap : 0))
                return fail(GROM_E_HIP, "device index build: the inflate launch failed");
            if (verify) {  // the piece's blocks against their CRC-32, before anything reads their bytes
                IXK(hipEventRecord(ev_crc, st));
                IXK(hipMemsetAsync(m32 + IX_CRC_WORD, 0, 4, st));
                IXK(hipMemsetAsync(m32 + IX_CRC_WORD + 1, 0xff, 4, st));
                if (dd_crc_launch(st, d_comp, p.comp_len, P<DdBlock>(dblk), p.nblk, Up, 0, ulen, P<uint8_t>(status),
                                  m32 + IX_CRC_WORD, m32 + 2, m32 + IX_CRC_WORD + 1))
                    return fail(GROM_E_HIP, "device index build: the CRC launch failed");
            }
            IXK(hipEventRecord(ev[1], st));
            IXK(hipMemsetAsync(P<uint32_t>(sub_n) + nsub, 0, 4, st));
            hipLaunchKernelGGL(k_ix_sub, dim3((unsigned)nch), dim3(IX_T), 0, st, Up, ulen, start, nsub, guess, n_ref,
                               P<int64_t>(sub_st), P<uint32_t>(sub_n), P<int64_t>(cg), P<int64_t>(cex), m32);
            hipLaunchKernelGGL(k_ix_chain, dim3(1), dim3(IX_T), 0, st, Up, ulen, start, nsub, nch, guess, n_ref,
                               P<int64_t>(sub_st), P<uint32_t>(sub_n), P<int64_t>(cg), P<int64_t>(cex), m32, m64);
            IXK(hipGetLastError());
            IXK(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, P<uint32_t>(sub_n), P<uint32_t>(sub_base), (int)(nsub + 1), st));
            IXK(hipEventRecord(ev[2], st));
            IXK(hipMemcpyAsync(h_small, misc.p, IX_MISC_BYTES, hipMemcpyDeviceToHost, st));
            IXK(hipMemcpyAsync(h_small + 16, P<uint32_t>(sub_base) + nsub, 4, hipMemcpyDeviceToHost, st));
            // the next piece is read and sent while this one is walked
            if ((rc = read_piece(s ^ 1)) != 0) return rc;
            IXK(hipStreamSynchronize(st));
            if (verify && ((const uint32_t *)h_small)[IX_CRC_WORD]) {  // a hard error, the block named
                const uint32_t bi = ((const uint32_t *)h_small)[IX_CRC_WORD + 1];
                const int64_t foff = p.c0 + ((int64_t)bi < p.nblk ? p.blk[(size_t)bi].c_off : 0);
                bgzf_crc_fail(path, foff);
                dd_crc_message(err, (int)sizeof(err), path, foff);
                return GROM_E_ARG;
            }
            if ((rc = check_bad((const uint32_t *)h_small)) != 0) return rc;
            const int64_t exit_pos = h_small[4];
            const int64_t R = (int64_t)(uint32_t)h_small[16];
            if (exit_pos < start || exit_pos > ulen) return fail(GROM_E_ARG, "device index build: the record chain broke");
            {
                float ms = 0;
                (void)hipEventElapsedTime(&ms, ev[0], verify ? ev_crc : ev[1]);
                ms_inflate += ms;
                if (verify) {
                    (void)hipEventElapsedTime(&ms, ev_crc, ev[1]);
                    ms_crc += ms;
                }
                (void)hipEventElapsedTime(&ms, ev[1], ev[2]);
                ms_walk += ms;
            }
            // ---- phase B: the records' facts, the reductions, the run list ----
            if (R > 0) {
                IXG(off, 8 * (size_t)R);
                IXG(tid, 4 * (size_t)R);
                IXG(pos, 4 * (size_t)R);
                IXG(end, 4 * (size_t)R);
                IXG(binu, 4 * (size_t)R);
                IXG(vbeg, 8 * (size_t)R);
                IXG(vend, 8 * (size_t)R);
                IXG(key, 8 * (size_t)(R + 1));
                IXG(pre, 8 * (size_t)(R + 1));
                size_t tb2 = 0;
                IXK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, (uint64_t *)nullptr, (uint64_t *)nullptr, (int)(R + 1), st));
                IXG(tmp, tb2);
                const unsigned gq = (unsigned)((nsub + 255) / 256), gr = (unsigned)((R + 255) / 256);
                IXK(hipEventRecord(ev[3], st));
                hipLaunchKernelGGL(k_ix_offsets, dim3(gq), dim3(256), 0, st, Up, ulen, start, nsub, P<int64_t>(sub_st),
                                   P<uint32_t>(sub_n), P<uint32_t>(sub_base), P<int64_t>(off), R, m32);
                hipLaunchKernelGGL(k_ix_facts, dim3(gr), dim3(256), 0, st, Up, ulen, P<int64_t>(off), R, P<int64_t>(tu),
                                   P<int64_t>(tc), nt, P<int32_t>(tid), P<int32_t>(pos), P<int32_t>(end), P<uint32_t>(binu),
                                   P<uint64_t>(vbeg), P<uint64_t>(vend), m32);
                IXK(hipMemsetAsync(P<uint64_t>(key) + R, 0, 8, st));
                hipLaunchKernelGGL(k_ix_reduce, dim3(gr), dim3(256), 0, st, R, P<int32_t>(tid), P<int32_t>(pos), P<int32_t>(end),
                                   P<uint32_t>(binu), P<uint64_t>(vbeg), n_ref, P<unsigned long long>(lin), P<int64_t>(lin_base),
                                   P<uint64_t>(key), m32, (unsigned long long *)(m64 + 1), dstate + 4 * (n_state & 1),
                                   dstate + 4 * ((n_state + 1) & 1));
                IXK(hipGetLastError());
                n_state++;
                IXK(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb2, P<uint64_t>(key), P<uint64_t>(pre), (int)(R + 1), st));
                IXK(hipMemcpyAsync(h_small, misc.p, IX_MISC_BYTES, hipMemcpyDeviceToHost, st));
                IXK(hipMemcpyAsync(h_small + 16, P<uint64_t>(pre) + R, 8, hipMemcpyDeviceToHost, st));
                IXK(hipStreamSynchronize(st));
                if ((rc = check_bad((const uint32_t *)h_small)) != 0) return rc;
                const int64_t nr = (int64_t)((uint64_t)h_small[16] >> 32);
                if (nr > 0) {
                    IXG(runs, sizeof(IxRun) * (size_t)nr);
                    hipLaunchKernelGGL(k_ix_runs, dim3(gr), dim3(256), 0, st, R, P<int32_t>(tid), P<uint32_t>(binu),
                                       P<uint64_t>(vbeg), P<uint64_t>(vend), P<uint64_t>(key), P<uint64_t>(pre), P<IxRun>(runs),
                                       nr, n_ref);
                    IXK(hipGetLastError());
                }
                IXK(hipEventRecord(ev[4], st));
                h_runs.resize((size_t)nr);
                if (nr > 0) IXK(hipMemcpyAsync(h_runs.data(), runs.p, sizeof(IxRun) * (size_t)nr, hipMemcpyDeviceToHost, st));
                IXK(hipStreamSynchronize(st));
                float ms = 0;
                (void)hipEventElapsedTime(&ms, ev[3], ev[4]);
                ms_reduce += ms;
                for (const IxRun &r : h_runs) {
                    if (r.tid < 0 || r.tid >= n_ref || r.j1 < r.j0 || r.u1 < r.u0)
                        return fail(GROM_E_ARG, "device index build: the run list is not whole");
                    push_run(r);
                }
                n_rec += R;
            }
            // the record that does not end in this piece goes to the next one
            origin += exit_pos;
            carry_pos = exit_pos;
            carry_len = ulen - exit_pos;
            start = 0;
            {
                size_t first = 0;
                while (first + 1 < keep.size() && keep[first + 1].abs_off < origin) first++;
                if (!keep.empty() && keep[first].abs_off >= origin) first = 0;
                keep.erase(keep.begin(), keep.begin() + (ptrdiff_t)first);
            }
            if (p.last) {
                if (carry_len != 0) return fail(GROM_E_ARG, "device index build: the BAM ends inside a record");
                break;
            }
        }
        flush_run();
        return 0;
    }

    // the file offset of the block after piece p
    int64_t foff_after(const PieceIn &p) const { return p.c0 + p.comp_len; }

    // the accumulators completed and written (under a temporary name)
    int write(const char *tmp_path) {
        const int64_t W = h_lin_base[(size_t)n_ref];
        std::vector<uint64_t> h_lin((size_t)std::max<int64_t>(W, 1));
        if (W > 0) IXK(hipMemcpy(h_lin.data(), lin.p, 8 * (size_t)W, hipMemcpyDeviceToHost));
        IXK(hipMemcpy(h_small, misc.p, IX_MISC_BYTES, hipMemcpyDeviceToHost));
        const uint64_t n_no_coor = (uint64_t)h_small[5];
        for (int32_t t = 0; t < n_ref; t++) {
            if (!any[(size_t)t]) continue;
            bai_racc_set_span(racc[(size_t)t], off_beg[(size_t)t], off_end[(size_t)t], n_map[(size_t)t], n_unm[(size_t)t]);
            const uint64_t *l = h_lin.data() + h_lin_base[(size_t)t];
            int64_t n = h_lin_base[(size_t)t + 1] - h_lin_base[(size_t)t];
            while (n > 0 && l[n - 1] == UINT64_MAX) n--;
            if (bai_racc_set_linear(racc[(size_t)t], l, (int32_t)n) != 0) return fail(GROM_E_NOMEM, "device index build: out of memory");
        }
        if (bai_write_racc(tmp_path, racc.data(), n_ref, n_no_coor, NULL, NULL) != 0)
            return fail(GROM_E_ARG, "device index build: cannot write the index file");
        return 0;
    }
};

}  // namespace

extern "C" int grom_bai_build_device(const char *bam_path, const char *bai_path, int device, int64_t out[8]) {
    const auto t0 = std::chrono::steady_clock::now();
    if (out) memset(out, 0, 8 * sizeof(int64_t));
    if (!bam_path) {
        grom_set_last_error("grom_bai_build_device: no BAM path");
        return GROM_E_ARG;
    }
    const std::string bai = bai_path ? std::string(bai_path) : std::string(bam_path) + ".bai";
    const std::string tmp = bai + ".tmp." + std::to_string((long long)getpid());
    int rc;
    {
        IxBuild B(bam_path);
        B.device = device;
        int64_t hdr_len = 0;
        bgzf_crc_error_clear();
        if (!B.in.fp || ix_read_header(bam_path, &hdr_len, B.ref_len) != 0) {
            char m[4400];
            snprintf(m, sizeof(m), "grom_bai_build_device: cannot read the BAM header of %s", bam_path);
            grom_set_last_error(bgzf_crc_error() ? bgzf_crc_error() : m);  // (a verifying reader names the damaged block)
            return GROM_E_ARG;
        }
        B.n_ref = (int32_t)B.ref_len.size();
        rc = B.run(hdr_len);
        if (rc == 0) rc = B.write(tmp.c_str());
        if (rc == 0 && rename(tmp.c_str(), bai.c_str()) != 0) rc = B.fail(GROM_E_ARG, "device index build: cannot rename the index file");
        if (rc != 0) {
            (void)remove(tmp.c_str());
            grom_set_last_error(B.err[0] ? B.err : "device index build failed");
        }
        const int64_t wall = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
        if (out) {
            out[0] = B.n_rec;
            out[1] = B.n_blk;
            out[2] = B.n_piece;
            out[3] = B.h_small ? (int64_t)((const uint32_t *)B.h_small)[3] : 0;
            out[4] = B.n_sub;
            out[5] = B.n_runs;
            out[6] = (int64_t)((B.ms_inflate + B.ms_walk + B.ms_reduce) * 1000.0);
            out[7] = wall;
        }
        if (getenv("GROM_VERBOSE"))
            fprintf(stderr, "grom: device index build: %lld records, %lld blocks, %lld pieces of <= %lld KB; inflate %.1f ms, "
                            "walk %.1f ms, reductions %.1f ms; wall %.1f ms\n",
                    (long long)B.n_rec, (long long)B.n_blk, (long long)B.n_piece, (long long)(B.piece_bytes >> 10),
                    B.ms_inflate, B.ms_walk, B.ms_reduce, wall / 1e3);
        if (getenv("GROM_VERBOSE") && B.verify)
            fprintf(stderr, "grom: device index build: block checksums %.1f ms (HIP events) next to the inflate's %.1f ms\n",
                    B.ms_crc, B.ms_inflate);
    }
    return rc;
}
