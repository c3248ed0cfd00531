// gzipdev.hip -- one plain gzip stream inflated on the device (DESIGN.md
// 4.7.1): the device side of gzipplan.h's read.  The compressed file is in
// HBM already (fastadev.hip's upload); the stages are
//   k_gz_guess    one wave per chunk of compressed bytes: the first bit that
//                 passes the strict dynamic-header test (a lane per byte)
//   k_gz_run      one lane per unit: counted (no stores), then -- for the
//                 units the chain took -- decoded into 16-bit symbols
//   k_gz_map      per group of units: the group's window map (symbols over the
//                 window before the group)
//   k_gz_windows  one workgroup: the window before every group
//   k_gz_resolve  per group: the symbols through the windows into the text,
//                 the window carried from unit to unit in LDS
//   k_gz_crc      a lane per 64 KB slice of the text, the table in LDS
// The per-lane code is gzipinf.h's, shared with the host twin (gzip_host.cpp).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/grom_amd.h"
#include "devbuf.h"
#include "gzipdev.h"
#include "gzipplan.h"

namespace {

#define GZ_LANES 64

__global__ void __launch_bounds__(GZ_LANES) k_gz_guess(const uint8_t *__restrict__ data, int64_t n, int64_t chunk,
                                                       int64_t nchunks, int mode, int64_t *__restrict__ out) {
    __shared__ uint32_t tab[GZ_PROBE_DWORDS * GZ_LANES];
    const int64_t c = blockIdx.x;
    if (c >= nchunks) return;
    const int lane = (int)threadIdx.x;
    const int64_t lo = c * chunk, hi = lo + chunk < n ? lo + chunk : n;
    int64_t found = -1;
    for (int64_t b0 = lo; b0 < hi; b0 += GZ_LANES) {
        const int64_t byte = b0 + lane;
        const int r = byte < hi ? gz_probe_byte<GZ_LANES>(data, n, byte, tab, lane) : -1;
        const unsigned long long hit = __ballot(r >= 0);
        if (hit) {
            const int first = __ffsll((long long)hit) - 1;
            found = (b0 + first) * 8 + __shfl(r, first);
            break;
        }
    }
    if (lane == 0) out[c] = found < 0 ? -1 : found + (mode == 2 ? 3 : 0);  // (mode 2: a start that is none)
}

template <bool WRITE>
__global__ void __launch_bounds__(GZ_LANES) k_gz_run(const uint8_t *__restrict__ data, int64_t n,
                                                     const GzJob *__restrict__ jobs, int64_t njobs, int64_t max_bits,
                                                     uint16_t *__restrict__ sym, GzRes *__restrict__ res) {
    __shared__ uint32_t tab[GI_LANE_DWORDS * GZ_LANES];
    const int64_t i = (int64_t)blockIdx.x * GZ_LANES + threadIdx.x;
    if (i >= njobs) return;
    GzRes r;
    gz_run<GZ_LANES, WRITE>(data, n, jobs[i], max_bits, sym, tab, (int)threadIdx.x, r);
    res[i] = r;
}

struct GzBlockCtx {
    __device__ __forceinline__ int tid() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int nt() const { return (int)blockDim.x; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

#define GZ_TPB 512

__global__ void __launch_bounds__(GZ_TPB) k_gz_map(const uint16_t *__restrict__ sym, const GzUnit *__restrict__ units,
                                                   int64_t nu, int64_t per, uint16_t *maps, uint16_t *tmp) {
    const int64_t g = blockIdx.x;
    const int64_t u0 = g * per, u1 = u0 + per < nu ? u0 + per : nu;
    gz_group_map(GzBlockCtx(), sym, units, u0, u1, maps + g * GZ_WIN, tmp + g * GZ_WIN);
}

__global__ void __launch_bounds__(1024) k_gz_windows(const uint16_t *__restrict__ maps, int64_t ngroups, uint8_t *win) {
    gz_group_windows(GzBlockCtx(), maps, ngroups, win);
}

__global__ void __launch_bounds__(GZ_TPB) k_gz_resolve(const uint16_t *__restrict__ sym, const GzUnit *__restrict__ units,
                                                       int64_t nu, int64_t per, const uint8_t *__restrict__ win,
                                                       uint8_t *__restrict__ text, uint32_t *err) {
    __shared__ uint8_t W[2][GZ_WIN];
    const int64_t g = blockIdx.x;
    const int64_t u0 = g * per, u1 = u0 + per < nu ? u0 + per : nu;
    gz_group_resolve(GzBlockCtx(), sym, units, u0, u1, win + g * GZ_WIN, W[0], W[1], text, err);
}

__global__ void __launch_bounds__(256) k_gz_crc(const uint8_t *__restrict__ text, const GzSlice *__restrict__ sl, int64_t n,
                                                uint32_t *__restrict__ out) {
    __shared__ uint32_t T[1024];
    for (int t = 0; t < 4; t++) {
        T[t * 256 + threadIdx.x] = gz_crc_entry(t, (int)threadIdx.x, T);
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = gz_crc_slice(text + sl[i].off, sl[i].len, T);
}

using Buf = DevBufOf<GROM_DEVCAT_DECODE, 256, true>;

#define GZK(x)                                                                                                      \
    do {                                                                                                            \
        hipError_t e_ = (x);                                                                                        \
        if (e_ != hipSuccess) {                                                                                     \
            snprintf(err, sizeof(err), "device gzip: HIP error %s at %s:%d", hipGetErrorString(e_), __FILE__, __LINE__); \
            return GROM_E_HIP;                                                                                      \
        }                                                                                                           \
    } while (0)
#define GZG(b, bytes)                                                                                               \
    do {                                                                                                            \
        if ((b).grow(bytes)) {                                                                                      \
            snprintf(err, sizeof(err), "device gzip: hipMalloc(%lld) failed", (long long)(bytes));                  \
            return GROM_E_NOMEM;                                                                                    \
        }                                                                                                           \
    } while (0)

struct DevBackend {
    hipStream_t st = nullptr;
    const uint8_t *data = nullptr;  // n bytes + GZ_PAD zeros
    int64_t n = 0, max_bits = 0;
    size_t text_pad = 0;
    uint8_t *text = nullptr;
    size_t text_cap = 0;
    Buf gbuf, jobs, res, sym, units, maps, tmp, win, flag, slices, crcs;
    hipEvent_t ev[GZ_STAGE_END + 1] = {};
    char err[512] = {0};

    ~DevBackend() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int64_t scratch() const {
        int64_t s = 0;
        for (const Buf *b : {&gbuf, &jobs, &res, &sym, &units, &maps, &tmp, &win, &flag, &slices, &crcs}) s += (int64_t)b->cap;
        return s;
    }
    // the stage that begins: an event between it and the one before
    void stage(int k) {
        if (k < 0 || k > GZ_STAGE_END) return;
        if (!ev[k] && hipEventCreate(&ev[k]) != hipSuccess) return;
        (void)hipEventRecord(ev[k], st);
    }
    int fetch(int64_t off, int k, uint8_t *dst) {
        if (off < 0 || off + k > n) return GROM_E_ARG;
        GZK(hipMemcpyAsync(dst, data + off, (size_t)k, hipMemcpyDeviceToHost, st));
        GZK(hipStreamSynchronize(st));
        return 0;
    }
    int guess(int64_t chunk, int mode, std::vector<int64_t> &g) {
        const int64_t nc = (n + chunk - 1) / chunk;
        if (nc <= 0) return 0;
        GZG(gbuf, 8 * (size_t)nc);
        hipLaunchKernelGGL(k_gz_guess, dim3((unsigned)nc), dim3(GZ_LANES), 0, st, data, n, chunk, nc, mode, P<int64_t>(gbuf));
        GZK(hipGetLastError());
        std::vector<int64_t> h((size_t)nc);
        GZK(hipMemcpyAsync(h.data(), gbuf.p, 8 * (size_t)nc, hipMemcpyDeviceToHost, st));
        GZK(hipStreamSynchronize(st));
        for (int64_t v : h)
            if (v >= 0) g.push_back(v);
        return 0;
    }
    template <bool WRITE>
    int run(const GzJob *j, int64_t k, GzRes *r) {
        GZG(jobs, sizeof(GzJob) * (size_t)k);
        GZG(res, sizeof(GzRes) * (size_t)k);
        GZK(hipMemcpyAsync(jobs.p, j, sizeof(GzJob) * (size_t)k, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_gz_run<WRITE>, dim3((unsigned)((k + GZ_LANES - 1) / GZ_LANES)), dim3(GZ_LANES), 0, st, data, n,
                           P<GzJob>(jobs), k, max_bits, P<uint16_t>(sym), P<GzRes>(res));
        GZK(hipGetLastError());
        GZK(hipMemcpyAsync(r, res.p, sizeof(GzRes) * (size_t)k, hipMemcpyDeviceToHost, st));
        GZK(hipStreamSynchronize(st));
        return 0;
    }
    int count(const GzJob *j, int64_t k, GzRes *r) { return run<false>(j, k, r); }
    int symbolic(const GzJob *j, int64_t k, GzRes *r) { return run<true>(j, k, r); }
    int alloc_text(int64_t total) {
        text_cap = (size_t)total + text_pad;
        if (grom_dev_malloc((void **)&text, text_cap, GROM_DEVCAT_DECODE) != 0) {
            text = nullptr;
            snprintf(err, sizeof(err), "device gzip: hipMalloc(%lld) failed", (long long)text_cap);
            return GROM_E_NOMEM;
        }
        GZG(sym, 2 * ((size_t)total + GZ_E));
        return 0;
    }
    int resolve(const GzUnit *u, int64_t nu, int64_t per, uint32_t *bad) {
        const int64_t ng = (nu + per - 1) / per;
        GZG(units, sizeof(GzUnit) * (size_t)nu);
        GZG(maps, 2 * (size_t)GZ_WIN * (size_t)ng);
        GZG(tmp, 2 * (size_t)GZ_WIN * (size_t)ng);
        GZG(win, (size_t)GZ_WIN * (size_t)ng);
        GZG(flag, 16);
        GZK(hipMemcpyAsync(units.p, u, sizeof(GzUnit) * (size_t)nu, hipMemcpyHostToDevice, st));
        GZK(hipMemsetAsync(flag.p, 0, 16, st));
        if (ng > 1)  // (nothing follows the last group)
            hipLaunchKernelGGL(k_gz_map, dim3((unsigned)(ng - 1)), dim3(GZ_TPB), 0, st, P<uint16_t>(sym), P<GzUnit>(units), nu,
                               per, P<uint16_t>(maps), P<uint16_t>(tmp));
        hipLaunchKernelGGL(k_gz_windows, dim3(1), dim3(1024), 0, st, P<uint16_t>(maps), ng, P<uint8_t>(win));
        GZK(hipGetLastError());
        stage(GZ_STAGE_RESOLVE);
        hipLaunchKernelGGL(k_gz_resolve, dim3((unsigned)ng), dim3(GZ_TPB), 0, st, P<uint16_t>(sym), P<GzUnit>(units), nu, per,
                           P<uint8_t>(win), text, P<uint32_t>(flag));
        GZK(hipGetLastError());
        GZK(hipMemcpyAsync(bad, flag.p, 4, hipMemcpyDeviceToHost, st));
        GZK(hipStreamSynchronize(st));
        return 0;
    }
    int crc(const GzSlice *s, int64_t k, uint32_t *out) {
        GZG(slices, sizeof(GzSlice) * (size_t)k);
        GZG(crcs, 4 * (size_t)k);
        GZK(hipMemcpyAsync(slices.p, s, sizeof(GzSlice) * (size_t)k, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_gz_crc, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, text, P<GzSlice>(slices), k,
                           P<uint32_t>(crcs));
        GZK(hipGetLastError());
        GZK(hipMemcpyAsync(out, crcs.p, 4 * (size_t)k, hipMemcpyDeviceToHost, st));
        GZK(hipStreamSynchronize(st));
        return 0;
    }
};

double env_kb(const char *name, double dflt) {
    const char *e = getenv(name);
    return e && atof(e) > 0 ? atof(e) : dflt;
}

}  // namespace

int gz_dev_read(hipStream_t st, const uint8_t *comp, int64_t n, size_t text_pad, uint8_t **text, size_t *text_cap,
                int64_t *size, int64_t stats[8], double ms[GZ_DEV_STAGES], char *err, size_t errn) {
    DevBackend b;
    b.st = st;
    b.data = comp;
    b.n = n;
    b.text_pad = text_pad;
    GzParams P;
    P.chunk_bytes = (int64_t)(env_kb("GROM_GZIP_CHUNK_KB", GZ_DEFAULT_CHUNK_KB) * 1024.0);
    P.unit_max_bytes = (int64_t)(env_kb("GROM_GZIP_UNIT_MAX_KB", GZ_DEFAULT_UNIT_MAX_KB) * 1024.0);
    const char *gm = getenv("GROM_GZIP_GUESS");
    P.guess_mode = gm ? atoi(gm) : 1;
    int64_t total = 0;
    char e2[512] = {0};
    int rc = gz_read(b, n, P, &total, stats, e2, sizeof(e2));
    stats[GZ_ST_SCRATCH] = b.scratch();
    if (rc == 0) {
        (void)hipStreamSynchronize(st);  // (the last stage's event)
        for (int k = 0; k < GZ_STAGE_END; k++) {
            float t = 0;
            if (b.ev[k] && b.ev[k + 1] && hipEventElapsedTime(&t, b.ev[k], b.ev[k + 1]) == hipSuccess) ms[k] = t;
        }
        *text = b.text;
        *text_cap = b.text_cap;
        *size = total;
        return 0;
    }
    if (b.text) grom_dev_free(b.text, b.text_cap, GROM_DEVCAT_DECODE);
    if (rc != GROM_FASTA_HOST_ONLY) snprintf(err, errn, "%s", b.err[0] ? b.err : (e2[0] ? e2 : "device gzip: the read failed"));
    return rc;
}
