// bgzfwrite.hip -- BGZF written on the device: the DEFLATE
// compressor's kernels (bgzfdef.h's phases, one BGZF block per wave), the
// piece pipeline and the writer behind grom_bgzf_writer_*, grom_bgzf_compress
// and grom_bgzf_blocks.  device = -1 runs the host twin (bgzfdef_host.cpp)
// through the same writer, so the file's bytes are the same either way.
//
// A piece is a whole number of 65280-byte payloads (the stream's end apart):
//   upload                      one copy from the pinned buffer being filled
//   k_bgzf_deflate              one wave per payload into its zeroed DF_SLOT-byte slot
//   k_bgzf_trailer              the payload's CRC-32 (bgzfcrc.h) and ISIZE behind it
//   k_bgzf_offsets              the prefix sum of the blocks' sizes
//   k_bgzf_gather               the slots packed, 16 bytes per lane, aligned on the destination
//   download                    the offsets, then the packed bytes once
// on the writer's own stream.  The kernels of one piece run while the caller
// fills the other pinned buffer; the packed bytes are fetched and written when
// the next piece is handed over (or at close).
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/grom_amd.h"
#include "bgzfcrc.h"
#include "bgzfdef.h"
#include "bgzfwrite.h"
#include "devbuf.h"

namespace {

using WBuf = DevBufOf<GROM_DEVCAT_OTHER, 256>;

#define BW_CRC_WAVES 4
#define BW_MAX_GRID 1024  // waves in flight: the token scratch is 255 KB per wave

// ---- one BGZF block per wave ----
__global__ void __launch_bounds__(DF_LANES) k_bgzf_deflate(const uint8_t *__restrict__ buf, const int64_t *__restrict__ offs,
                                                           int64_t n_blk, uint8_t *__restrict__ slots,
                                                           uint32_t *__restrict__ tok_all, uint32_t *__restrict__ sizes,
                                                           uint32_t *__restrict__ kinds) {
    __shared__ DfShared S;
    const int lane = (int)threadIdx.x;
    uint32_t *tok = tok_all + (size_t)blockIdx.x * DF_MAX_PAYLOAD;
    for (int64_t j = blockIdx.x; j < n_blk; j += gridDim.x) {
        const int64_t o = offs[j], len = offs[j + 1] - o;
        uint32_t *out = reinterpret_cast<uint32_t *>(slots + (size_t)j * DF_SLOT);
        if (len < 0 || len > DF_MAX_PAYLOAD) {  // (the host checked; a slot is never overrun)
            if (lane == 0) { sizes[j] = 0; kinds[j] = 0xffu; }
            continue;
        }
        const uint8_t *in = buf + o;
        const uint32_t n = (uint32_t)len;
        __syncthreads();  // (the last block's state is no longer read)
        df_init(&S, lane);
        __syncthreads();
        for (uint32_t base = 0; base < n; base += DF_LANES) {
            df_match(&S, in, n, base, lane);
            __syncthreads();
            df_insert(&S, in, n, base, lane);
            if (lane == 0) df_parse(&S, in, n, base, tok);
            __syncthreads();
        }
        if (lane == 0) df_plan(&S, n, out);
        __syncthreads();
        const int kind = S.kind;
        if (kind == DF_STORED) {
            uint8_t *o8 = reinterpret_cast<uint8_t *>(out) + (S.body_bit >> 3);
            for (uint32_t i = (uint32_t)lane; i < n; i += DF_LANES) o8[i] = in[i];
        } else {
            const DfCode *C = &S.code[kind == DF_LITDYN ? 1 : 0];
            const uint32_t nt = kind == DF_LITDYN ? n : S.ntok;
            uint32_t bp = S.body_bit;
            for (uint32_t t0 = 0; t0 < nt; t0 += DF_LANES) {
                const uint32_t t = t0 + (uint32_t)lane;
                uint32_t v0 = 0, n0 = 0, v1 = 0, n1 = 0;
                if (t < nt) df_token_bits(C, kind == DF_LITDYN ? (uint32_t)in[t] : tok[t], v0, n0, v1, n1);
                uint32_t incl = n0 + n1;  // the wave's inclusive prefix sum
#pragma unroll
                for (int d = 1; d < DF_LANES; d <<= 1) {
                    const uint32_t up = (uint32_t)__shfl_up((int)incl, d, DF_LANES);
                    if (lane >= d) incl += up;
                }
                const uint32_t at = bp + incl - (n0 + n1);
                df_put(out, at, v0, n0);
                df_put(out, at + n0, v1, n1);
                bp += (uint32_t)__shfl((int)incl, DF_LANES - 1, DF_LANES);
            }
            if (lane == 0) df_put(out, bp, C->lcode[256], C->llen[256]);
        }
        if (lane == 0) {
            sizes[j] = 18 + S.cbytes + 8;
            kinds[j] = (uint32_t)kind;
        }
    }
}

// ---- the trailer: CRC-32 of the payload (k_bgzf_crc's arithmetic), ISIZE ----
__global__ void __launch_bounds__(BW_CRC_WAVES *BC_LANES) k_bgzf_trailer(const uint8_t *__restrict__ buf, int64_t buf_cap,
                                                                         const int64_t *__restrict__ offs, int64_t n_blk,
                                                                         uint8_t *__restrict__ slots,
                                                                         const uint32_t *__restrict__ sizes) {
    __shared__ uint32_t tab[BC_DWORDS];
    for (int s = 0; s < BC_STAGES; s++) {
        bc_build_stage(s, (int)threadIdx.x, BW_CRC_WAVES * BC_LANES, tab);
        __syncthreads();
    }
    const int lane = (int)threadIdx.x & (BC_LANES - 1), wave = (int)threadIdx.x / BC_LANES;
    for (int64_t j = (int64_t)blockIdx.x * BW_CRC_WAVES + wave; j < n_blk; j += (int64_t)gridDim.x * BW_CRC_WAVES) {
        const int64_t o = offs[j], len = offs[j + 1] - o;
        const uint32_t size = sizes[j];
        if (size < 26 || size > DF_MAX_PAYLOAD + 31 || len < 0 || len > DF_MAX_PAYLOAD || o < 0 || o + len > buf_cap) continue;
        const uint32_t n = (uint32_t)len;
        uint32_t v = n ? bc_lane(buf, buf_cap, o, n, lane, tab) : 0u;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v ^= (uint32_t)__shfl_xor((int)v, d, 64);
        if (lane == 0) df_trailer(slots + (size_t)j * DF_SLOT, size, bc_combine(v, buf, buf_cap, o, n, tab), n);
    }
}

// ---- ooff[0..n_blk]: the exclusive prefix sum of the sizes (one workgroup) ----
__global__ void __launch_bounds__(256) k_bgzf_offsets(const uint32_t *__restrict__ sizes, int64_t n_blk,
                                                      int64_t *__restrict__ ooff) {
    __shared__ int64_t part[256];
    const int t = (int)threadIdx.x;
    const int64_t per = (n_blk + 255) / 256, a = t * per < n_blk ? t * per : n_blk, b = a + per < n_blk ? a + per : n_blk;
    int64_t s = 0;
    for (int64_t i = a; i < b; i++) s += sizes[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int i = 0; i < 256; i++) {
            const int64_t v = part[i];
            part[i] = run;
            run += v;
        }
        ooff[n_blk] = run;
    }
    __syncthreads();
    s = part[t];
    for (int64_t i = a; i < b; i++) {
        ooff[i] = s;
        s += sizes[i];
    }
}

// ---- the slots packed: one workgroup per block, 16-byte stores aligned on dst ----
__global__ void __launch_bounds__(256) k_bgzf_gather(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ sizes,
                                                     const int64_t *__restrict__ ooff, int64_t n_blk,
                                                     uint8_t *__restrict__ dst, int64_t dst_cap) {
    const uint32_t tid = threadIdx.x;
    for (int64_t j = blockIdx.x; j < n_blk; j += gridDim.x) {
        const uint8_t *s = slots + (size_t)j * DF_SLOT;  // (16-byte aligned)
        const uint32_t size = sizes[j];
        const int64_t D = ooff[j];
        if (size > DF_MAX_PAYLOAD + 31 || D < 0 || D + (int64_t)size > dst_cap) continue;
        uint32_t head = (uint32_t)((0 - D) & 15);
        if (head > size) head = size;
        if (tid < head) dst[D + tid] = s[tid];
        const uint32_t nw = (size - head) >> 4;
        const uint4 *sw = reinterpret_cast<const uint4 *>(s);
        uint4 *dw = reinterpret_cast<uint4 *>(dst + D + head);
        const uint32_t ws = head >> 2, bs = 8 * (head & 3);
        for (uint32_t k = tid; k < nw; k += 256) {
            // the source bytes [head + 16 k, head + 16 k + 16) out of two aligned words (the slot has 16 spare bytes)
            const uint4 lo = sw[k], hi = sw[k + 1];
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
        for (uint32_t i = head + 16 * nw + tid; i < size; i += 256) dst[D + i] = s[i];
    }
}

const uint8_t EOF_BLOCK[28] = {0x1f, 0x8b, 0x08, 0x04, 0x00, 0x00, 0x00, 0x00, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43,
                               0x02, 0x00, 0x1b, 0x00, 0x03, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00};

#define BWK(x)                                                                                                   \
    do {                                                                                                         \
        hipError_t e_ = (x);                                                                                     \
        if (e_ != hipSuccess) {                                                                                  \
            snprintf(err, sizeof(err), "BGZF write: HIP error %s at %s:%d", hipGetErrorString(e_), __FILE__, __LINE__); \
            return GROM_E_HIP;                                                                                   \
        }                                                                                                        \
    } while (0)
#define BWG(b, bytes)                                                                                  \
    do {                                                                                               \
        if ((b).grow(bytes)) {                                                                         \
            snprintf(err, sizeof(err), "BGZF write: hipMalloc(%lld) failed", (long long)(bytes));      \
            return GROM_E_NOMEM;                                                                       \
        }                                                                                              \
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

// the device side of one set of payloads: buffers, stream, launches
struct BwDevice {
    int device = -1;
    hipStream_t st = nullptr;
    hipEvent_t ev[2] = {};
    WBuf in, offs, slots, tok, sizes, kinds, ooff, dst;
    int64_t dst_cap = 0;
    char err[512] = {0};

    ~BwDevice() { close(); }
    void close() {
        if (device < 0) return;
        DevGuard g(device);
        if (st) (void)hipStreamSynchronize(st);
        for (hipEvent_t &e : ev)
            if (e) { (void)hipEventDestroy(e); e = nullptr; }
        if (st) (void)hipStreamDestroy(st);
        st = nullptr;
        for (WBuf *b : {&in, &offs, &slots, &tok, &sizes, &kinds, &ooff, &dst}) b->release();
        device = -1;
    }
    int open(int dev) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || dev < 0 || dev >= ndev) {
            snprintf(err, sizeof(err), "BGZF write: no device %d (%d visible)", dev, ndev);
            return GROM_E_NODEV;
        }
        DevGuard g(dev);
        if (!g.ok) {
            snprintf(err, sizeof(err), "BGZF write: device %d cannot be used", dev);
            return GROM_E_NODEV;
        }
        device = dev;
        BWK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        for (hipEvent_t &e : ev) BWK(hipEventCreate(&e));
        return 0;
    }
    // room for n_blk payloads of in_bytes in all
    int reserve(int64_t in_bytes, int64_t n_blk) {
        const int64_t grid = std::min<int64_t>(std::max<int64_t>(n_blk, 1), BW_MAX_GRID);
        BWG(in, (size_t)in_bytes + 64);
        BWG(offs, sizeof(int64_t) * (size_t)(n_blk + 1));
        BWG(slots, (size_t)std::max<int64_t>(n_blk, 1) * DF_SLOT);
        BWG(tok, (size_t)grid * DF_MAX_PAYLOAD * sizeof(uint32_t));  // (by the waves in flight, not by the blocks)
        BWG(sizes, sizeof(uint32_t) * (size_t)(n_blk + 1));
        BWG(kinds, sizeof(uint32_t) * (size_t)(n_blk + 1));
        BWG(ooff, sizeof(int64_t) * (size_t)(n_blk + 1));
        dst_cap = in_bytes + 32 * n_blk + 64;
        BWG(dst, (size_t)dst_cap);
        return 0;
    }
    // h_in[0, in_bytes) and h_offs[0..n_blk] (host memory that stays until wait()) uploaded and compressed;
    // h_ooff[0..n_blk] and h_kinds[0..n_blk) come back on the stream
    int launch(const uint8_t *h_in, int64_t in_bytes, const int64_t *h_offs, int64_t n_blk, int64_t *h_ooff,
               uint32_t *h_kinds) {
        DevGuard g(device);
        int rc = reserve(in_bytes, n_blk);
        if (rc) return rc;
        if (in_bytes) BWK(hipMemcpyAsync(in.p, h_in, (size_t)in_bytes, hipMemcpyHostToDevice, st));
        BWK(hipMemcpyAsync(offs.p, h_offs, sizeof(int64_t) * (size_t)(n_blk + 1), hipMemcpyHostToDevice, st));
        BWK(hipEventRecord(ev[0], st));
        if (n_blk > 0) {
            BWK(hipMemsetAsync(slots.p, 0, (size_t)n_blk * DF_SLOT, st));
            const unsigned grid = (unsigned)std::min<int64_t>(n_blk, BW_MAX_GRID);
            hipLaunchKernelGGL(k_bgzf_deflate, dim3(grid), dim3(DF_LANES), 0, st, P<uint8_t>(in), P<int64_t>(offs), n_blk,
                               P<uint8_t>(slots), P<uint32_t>(tok), P<uint32_t>(sizes), P<uint32_t>(kinds));
            const unsigned cgrid = (unsigned)std::min<int64_t>((n_blk + BW_CRC_WAVES - 1) / BW_CRC_WAVES, 1024);
            hipLaunchKernelGGL(k_bgzf_trailer, dim3(cgrid), dim3(BW_CRC_WAVES * BC_LANES), 0, st, P<uint8_t>(in), in_bytes,
                               P<int64_t>(offs), n_blk, P<uint8_t>(slots), P<uint32_t>(sizes));
        }
        hipLaunchKernelGGL(k_bgzf_offsets, dim3(1), dim3(256), 0, st, P<uint32_t>(sizes), n_blk, P<int64_t>(ooff));
        if (n_blk > 0)
            hipLaunchKernelGGL(k_bgzf_gather, dim3((unsigned)std::min<int64_t>(n_blk, 65535)), dim3(256), 0, st,
                               P<uint8_t>(slots), P<uint32_t>(sizes), P<int64_t>(ooff), n_blk, P<uint8_t>(dst), dst_cap);
        BWK(hipGetLastError());
        BWK(hipEventRecord(ev[1], st));
        BWK(hipMemcpyAsync(h_ooff, ooff.p, sizeof(int64_t) * (size_t)(n_blk + 1), hipMemcpyDeviceToHost, st));
        if (n_blk > 0) BWK(hipMemcpyAsync(h_kinds, kinds.p, sizeof(uint32_t) * (size_t)n_blk, hipMemcpyDeviceToHost, st));
        return 0;
    }
    // the launch finished (its tables are on the host); *us += the kernels' time
    int wait(int64_t *us) {
        DevGuard g(device);
        BWK(hipStreamSynchronize(st));
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess && us) *us += (int64_t)(ms * 1000.0f) + 1;
        return 0;
    }
    // its packed bytes (h_ooff[n_blk] of them) copied to h_dst
    int fetch(int64_t total, uint8_t *h_dst, int64_t h_cap) {
        if (total < 0 || total > dst_cap || total > h_cap) {
            snprintf(err, sizeof(err), "BGZF write: %lld packed bytes do not fit (%lld)", (long long)total, (long long)h_cap);
            return GROM_E_HIP;
        }
        DevGuard g(device);
        if (total) BWK(hipMemcpyAsync(h_dst, dst.p, (size_t)total, hipMemcpyDeviceToHost, st));
        BWK(hipStreamSynchronize(st));
        return 0;
    }
};

int64_t piece_payloads() {
    const char *e = getenv("GROM_BGZF_PIECE_KB");
    int64_t bytes = (int64_t)1024 * DF_MAX_PAYLOAD;  // 63.75 MB: one payload per wave in flight
    if (e && atof(e) > 0) bytes = (int64_t)(atof(e) * 1024.0);
    return std::max<int64_t>(1, std::min<int64_t>(bytes / DF_MAX_PAYLOAD, 16384));
}

}  // namespace

// ---- the writer ----
struct grom_bgzf_writer {
    std::string path, tmp, gzi;
    FILE *fp = nullptr;
    int device = -1;
    BwDevice dev;
    int64_t piece = 0;  // bytes per piece: a whole number of payloads
    uint8_t *h_in[2] = {nullptr, nullptr}, *h_out = nullptr;  // pinned with a device, else malloc
    int64_t out_cap = 0, fill = 0;
    int cur = 0;
    std::vector<int64_t> h_offs[2], v_ooff;
    int64_t *h_ooff = nullptr;   // the finished piece's block offsets and kinds (pinned with a device: the copies
    uint32_t *h_kinds = nullptr; // back must not wait on the host)
    int64_t flying = -1;  // the blocks of the piece on the device, -1: none
    std::vector<uint64_t> index;  // (compressed, uncompressed) of every block after the first
    int64_t n_blk = 0, kinds[4] = {0, 0, 0, 0}, in_bytes = 0, out_bytes = 0, pieces = 0, device_us = 0;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    int failed = 0;
    char err[4400] = {0};

    int fail(int code, const char *m) {
        if (!failed) {
            failed = code;
            snprintf(err, sizeof(err), "%s", m);
        }
        return failed;
    }
    void free_host() {
        for (uint8_t *&p : h_in) {
            if (p && device >= 0) (void)hipHostFree(p);
            else free(p);
            p = nullptr;
        }
        if (h_out && device >= 0) (void)hipHostFree(h_out);
        else free(h_out);
        h_out = nullptr;
        if (h_ooff && device >= 0) (void)hipHostFree(h_ooff);
        h_ooff = nullptr;
    }
    // the blocks of a finished piece: the index's pairs, the file
    int take(int64_t nb, const int64_t *uoffs, const int64_t k4[4]) {
        const int64_t total = h_ooff[(size_t)nb];
        for (int64_t i = 0; i < nb; i++)
            if (n_blk + i > 0) {
                index.push_back((uint64_t)(out_bytes + h_ooff[(size_t)i]));
                index.push_back((uint64_t)(in_bytes + uoffs[i]));
            }
        for (int k = 0; k < 4; k++) kinds[k] += k4[k];
        if (total && fwrite(h_out, 1, (size_t)total, fp) != (size_t)total) return fail(GROM_E_ARG, "BGZF write: write error");
        n_blk += nb;
        in_bytes += uoffs[nb];
        out_bytes += total;
        pieces++;
        return 0;
    }
    int finish_flying() {
        if (flying < 0) return 0;
        const int64_t nb = flying;
        const int s = cur ^ 1;  // (the buffer handed over last)
        flying = -1;
        if (dev.wait(&device_us)) return fail(GROM_E_HIP, dev.err);
        int64_t k4[4] = {0, 0, 0, 0};
        for (int64_t i = 0; i < nb; i++) {
            if (h_kinds[(size_t)i] > 3) return fail(GROM_E_HIP, "BGZF write: a payload was not compressed");
            k4[h_kinds[(size_t)i]]++;
        }
        if (dev.fetch(h_ooff[(size_t)nb], h_out, out_cap)) return fail(GROM_E_HIP, dev.err);
        return take(nb, h_offs[s].data(), k4);
    }
    // the filled part of the current buffer goes out as one piece
    int flush() {
        if (failed) return failed;
        if (fill == 0) return 0;
        const int64_t nb = (fill + DF_MAX_PAYLOAD - 1) / DF_MAX_PAYLOAD;
        std::vector<int64_t> &uo = h_offs[cur];
        uo.resize((size_t)nb + 1);
        for (int64_t i = 0; i <= nb; i++) uo[(size_t)i] = std::min<int64_t>(i * DF_MAX_PAYLOAD, fill);
        if (device < 0) {
            v_ooff.resize((size_t)nb + 1);
            h_ooff = v_ooff.data();
            int64_t k4[4] = {0, 0, 0, 0};
            if (df_host_blocks(h_in[cur], uo.data(), nb, h_out, out_cap, h_ooff, k4) != 0)
                return fail(GROM_E_ARG, "BGZF write: the host compressor failed");
            const int rc = take(nb, uo.data(), k4);
            fill = 0;
            return rc;
        }
        int rc = finish_flying();
        if (rc) return rc;
        if (dev.launch(h_in[cur], fill, uo.data(), nb, h_ooff, h_kinds)) return fail(GROM_E_HIP, dev.err);
        flying = nb;
        cur ^= 1;
        fill = 0;
        return 0;
    }
};

extern "C" grom_bgzf_writer *grom_bgzf_writer_open(const char *path, int device, const char *gzi_path) {
    if (!path) {
        grom_set_last_error("BGZF write: no path");
        return nullptr;
    }
    grom_bgzf_writer *w = new grom_bgzf_writer;
    w->path = path;
    w->tmp = w->path + ".tmp." + std::to_string((long long)getpid());
    if (gzi_path) w->gzi = gzi_path;
    w->device = device < 0 ? -1 : device;
    w->piece = piece_payloads() * DF_MAX_PAYLOAD;
    w->out_cap = w->piece + 32 * (w->piece / DF_MAX_PAYLOAD) + 64;
    char m[4600];
    if (w->device >= 0 && w->dev.open(w->device) != 0) {
        grom_set_last_error(w->dev.err);
        w->device = -1;
        delete w;
        return nullptr;
    }
    bool ok = true;
    if (w->device >= 0) {
        for (uint8_t *&p : w->h_in) ok = ok && hipHostMalloc((void **)&p, (size_t)w->piece, hipHostMallocDefault) == hipSuccess;
        ok = ok && hipHostMalloc((void **)&w->h_out, (size_t)w->out_cap, hipHostMallocDefault) == hipSuccess;
        const size_t max_nb = (size_t)(w->piece / DF_MAX_PAYLOAD);
        ok = ok && hipHostMalloc((void **)&w->h_ooff, (max_nb + 2) * 12, hipHostMallocDefault) == hipSuccess;
        if (ok) w->h_kinds = (uint32_t *)(w->h_ooff + max_nb + 2);
    } else {
        ok = (w->h_in[0] = (uint8_t *)malloc((size_t)w->piece)) != nullptr &&
             (w->h_out = (uint8_t *)malloc((size_t)w->out_cap)) != nullptr;
    }
    if (ok) w->fp = fopen(w->tmp.c_str(), "wb");
    if (!ok || !w->fp) {
        snprintf(m, sizeof(m), ok ? "BGZF write: cannot open %s" : "BGZF write: out of memory (%s)", path);
        grom_set_last_error(m);
        w->free_host();
        delete w;
        return nullptr;
    }
    return w;
}

extern "C" int grom_bgzf_writer_write(grom_bgzf_writer *w, const void *buf, int64_t n) {
    if (!w || n < 0 || (n > 0 && !buf)) {
        grom_set_last_error("BGZF write: bad arguments");
        return GROM_E_ARG;
    }
    const uint8_t *p = (const uint8_t *)buf;
    while (n > 0 && !w->failed) {
        const int64_t k = std::min<int64_t>(n, w->piece - w->fill);
        memcpy(w->h_in[w->cur] + w->fill, p, (size_t)k);
        w->fill += k;
        p += k;
        n -= k;
        if (w->fill == w->piece) w->flush();
    }
    if (w->failed) grom_set_last_error(w->err);
    return w->failed;
}

extern "C" int grom_bgzf_writer_close(grom_bgzf_writer *w, int64_t out[10]) {
    if (!w) return GROM_E_ARG;
    w->flush();  // (the tail: under a piece, its last payload under 65280 bytes)
    w->finish_flying();
    if (!w->failed && fwrite(EOF_BLOCK, 1, 28, w->fp) != 28) w->fail(GROM_E_ARG, "BGZF write: write error");
    if (!w->failed) w->out_bytes += 28;
    if (w->fp && fclose(w->fp) != 0) w->fail(GROM_E_ARG, "BGZF write: write error at close");
    w->fp = nullptr;
    const std::string gtmp = w->gzi.empty() ? std::string() : w->gzi + ".tmp." + std::to_string((long long)getpid());
    if (!w->failed && !w->gzi.empty()) {
        // bgzip's .gzi: the number of entries, then (compressed offset, uncompressed offset) of every block after the first
        FILE *g = fopen(gtmp.c_str(), "wb");
        const uint64_t cnt = w->index.size() / 2;
        if (!g || fwrite(&cnt, 8, 1, g) != 1 || (cnt && fwrite(w->index.data(), 16, (size_t)cnt, g) != (size_t)cnt))
            w->fail(GROM_E_ARG, "BGZF write: cannot write the .gzi index");
        if (g && fclose(g) != 0) w->fail(GROM_E_ARG, "BGZF write: cannot write the .gzi index");
    }
    if (!w->failed && rename(w->tmp.c_str(), w->path.c_str()) != 0) w->fail(GROM_E_ARG, "BGZF write: cannot rename the file");
    if (!w->failed && !w->gzi.empty() && rename(gtmp.c_str(), w->gzi.c_str()) != 0)
        w->fail(GROM_E_ARG, "BGZF write: cannot rename the .gzi index");
    if (w->failed) {
        (void)remove(w->tmp.c_str());
        if (!gtmp.empty()) (void)remove(gtmp.c_str());
        grom_set_last_error(w->err);
    }
    if (out) {
        out[0] = w->n_blk;
        for (int k = 0; k < 4; k++) out[1 + k] = w->kinds[k];
        out[5] = w->in_bytes;
        out[6] = w->out_bytes;
        out[7] = w->pieces;
        out[8] = w->device_us;
        out[9] = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - w->t0).count();
    }
    const int rc = w->failed;
    w->dev.close();  // (the device memory is freed here, not at the process's exit)
    w->free_host();
    delete w;
    return rc;
}

extern "C" int64_t grom_bgzf_writer_block_offsets(grom_bgzf_writer *w, int64_t *coff, int64_t cap) {
    if (!w || !coff) return GROM_E_ARG;
    w->flush();
    w->finish_flying();
    if (w->failed) {
        grom_set_last_error(w->err);
        return w->failed;
    }
    if (cap < w->n_blk + 1) return GROM_E_ARG;
    for (int64_t i = 0; i < w->n_blk; i++) coff[i] = i == 0 ? 0 : (int64_t)w->index[(size_t)(2 * (i - 1))];
    coff[w->n_blk] = w->out_bytes;
    return w->n_blk;
}

extern "C" int grom_bgzf_compress(const char *src, const char *dst, int device, int64_t out[10]) {
    if (out) memset(out, 0, 10 * sizeof(int64_t));
    char m[4600];
    FILE *fp = src ? fopen(src, "rb") : nullptr;
    if (!fp || !dst) {
        snprintf(m, sizeof(m), "BGZF write: cannot open %s", src ? src : "(no path)");
        grom_set_last_error(m);
        if (fp) fclose(fp);
        return GROM_E_ARG;
    }
    const std::string gzi = std::string(dst) + ".gzi";
    grom_bgzf_writer *w = grom_bgzf_writer_open(dst, device, gzi.c_str());
    if (!w) {
        fclose(fp);
        return device >= 0 ? GROM_E_NODEV : GROM_E_ARG;
    }
    // read straight into the (pinned) buffer being filled
    int rc = 0;
    for (;;) {
        const size_t got = fread(w->h_in[w->cur] + w->fill, 1, (size_t)(w->piece - w->fill), fp);
        if (got == 0) break;
        w->fill += (int64_t)got;
        if (w->fill == w->piece && (rc = w->flush()) != 0) break;
    }
    if (ferror(fp)) w->fail(GROM_E_ARG, "BGZF write: read error");
    fclose(fp);
    rc = grom_bgzf_writer_close(w, out);
    return rc;
}

extern "C" int grom_bgzf_blocks(const uint8_t *buf, const int64_t *offs, int64_t n_blk, int device, uint8_t *dst,
                                int64_t dst_cap, int64_t *dst_offs) {
    if (!offs || n_blk < 0 || !dst || !dst_offs || (n_blk > 0 && !buf && offs[n_blk] > 0)) {
        grom_set_last_error("BGZF blocks: bad arguments");
        return GROM_E_ARG;
    }
    for (int64_t i = 0; i < n_blk; i++)
        if (offs[i] < 0 || offs[i + 1] < offs[i] || offs[i + 1] - offs[i] > DF_MAX_PAYLOAD) {
            grom_set_last_error("BGZF blocks: a payload of more than 65280 bytes, or offsets that decrease");
            return GROM_E_ARG;
        }
    if (device < 0) {
        const int rc = df_host_blocks(buf, offs, n_blk, dst, dst_cap, dst_offs, nullptr);
        if (rc) grom_set_last_error(rc == -2 ? "BGZF blocks: dst is too small" : "BGZF blocks: the host compressor failed");
        return rc ? GROM_E_ARG : 0;
    }
    BwDevice D;
    if (D.open(device) != 0) {
        grom_set_last_error(D.err);
        return GROM_E_NODEV;
    }
    std::vector<uint32_t> kinds((size_t)n_blk + 1);
    int64_t us = 0;
    // (dst is filled only when everything fits: the offsets come first)
    int rc = D.launch(buf, n_blk ? offs[n_blk] : 0, offs, n_blk, dst_offs, kinds.data());
    if (rc == 0) rc = D.wait(&us);
    if (rc == 0 && dst_offs[n_blk] > dst_cap) {
        grom_set_last_error("BGZF blocks: dst is too small");
        return GROM_E_ARG;
    }
    if (rc == 0) rc = D.fetch(dst_offs[n_blk], dst, dst_cap);
    if (rc) grom_set_last_error(D.err);
    return rc;
}
