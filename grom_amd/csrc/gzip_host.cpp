// gzip_host.cpp -- the host twin of the device's parallel gzip read
// (gzipdev.hip): the same guess, count/verify, symbolic
// decode, window hand-over, resolve and CRC code (gzipinf.h, gzipplan.h) run
// with one lane in loops.  Checked against zlib by tests/test_gzip_host.py and
// under sanitizers by tools/gzip_check.cpp.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/grom_amd.h"
#include "gzipplan.h"

namespace {

struct HostBackend {
    const uint8_t *in = nullptr;  // n bytes + GZ_PAD zeros
    int64_t n = 0;
    int64_t max_bits = 0;
    std::vector<uint16_t> sym;
    std::vector<uint8_t> text;
    uint32_t tab[GI_LANE_DWORDS];
    int64_t scratch = 0;

    void stage(int) {}
    int fetch(int64_t off, int k, uint8_t *dst) {
        if (off < 0 || off + k > n) return GROM_E_ARG;
        memcpy(dst, in + off, (size_t)k);
        return 0;
    }
    int guess(int64_t chunk, int mode, std::vector<int64_t> &g) {
        for (int64_t c0 = 0; c0 < n; c0 += chunk) {
            const int64_t hi = std::min<int64_t>(n, c0 + chunk);
            for (int64_t byte = c0; byte < hi; byte++) {
                const int r = gz_probe_byte<1>(in, n, byte, tab, 0);
                if (r >= 0) {
                    g.push_back(byte * 8 + r + (mode == 2 ? 3 : 0));  // (mode 2: a start that is none)
                    break;
                }
            }
        }
        return 0;
    }
    int count(const GzJob *jobs, int64_t k, GzRes *res) {
        for (int64_t i = 0; i < k; i++) gz_run<1, false>(in, n, jobs[i], max_bits, nullptr, tab, 0, res[i]);
        return 0;
    }
    int alloc_text(int64_t total) {
        sym.assign((size_t)total + GZ_E, 0);
        text.assign((size_t)total + GZ_E, 0);
        scratch += 2 * (total + GZ_E);
        return 0;
    }
    int symbolic(const GzJob *jobs, int64_t k, GzRes *res) {
        for (int64_t i = 0; i < k; i++) gz_run<1, true>(in, n, jobs[i], max_bits, sym.data(), tab, 0, res[i]);
        return 0;
    }
    int resolve(const GzUnit *units, int64_t nu, int64_t per, uint32_t *bad) {
        const int64_t ngr = (nu + per - 1) / per;
        std::vector<uint16_t> maps((size_t)ngr * GZ_WIN), tmp(GZ_WIN);
        std::vector<uint8_t> win((size_t)ngr * GZ_WIN), w0(GZ_WIN), w1(GZ_WIN);
        scratch += (int64_t)ngr * GZ_WIN * 3;
        const GzOneLane lane;
        for (int64_t gr = 0; gr + 1 < ngr; gr++)  // (nothing follows the last group)
            gz_group_map(lane, sym.data(), units, gr * per, std::min(nu, gr * per + per), maps.data() + gr * GZ_WIN,
                         tmp.data());
        gz_group_windows(lane, maps.data(), ngr, win.data());
        for (int64_t gr = 0; gr < ngr; gr++)
            gz_group_resolve(lane, sym.data(), units, gr * per, std::min(nu, gr * per + per), win.data() + gr * GZ_WIN,
                             w0.data(), w1.data(), text.data(), bad);
        return 0;
    }
    int crc(const GzSlice *sl, int64_t k, uint32_t *out) {
        static uint32_t T[1024];
        static bool have = false;
        if (!have) {
            for (int t = 0; t < 4; t++)
                for (int i = 0; i < 256; i++) T[t * 256 + i] = gz_crc_entry(t, i, T);
            have = true;
        }
        for (int64_t i = 0; i < k; i++) out[i] = gz_crc_slice(text.data() + sl[i].off, sl[i].len, T);
        return 0;
    }
};

}  // namespace

extern "C" int grom_gzip_inflate_host(const uint8_t *in, int64_t n, int64_t chunk_bytes, int64_t unit_max_bytes,
                                      int guess_mode, uint8_t **out, int64_t *out_len, int64_t stats[8]) {
    if (out) *out = nullptr;
    if (out_len) *out_len = 0;
    int64_t st[8];
    if (!in || n < 0 || !out || !out_len) {
        grom_set_last_error("grom_gzip_inflate_host: bad argument");
        return GROM_E_ARG;
    }
    std::vector<uint8_t> copy((size_t)n + GZ_PAD + 8, 0);  // (the reader looks ahead: zeros after the data)
    memcpy(copy.data(), in, (size_t)n);
    HostBackend b;
    b.in = copy.data();
    b.n = n;
    GzParams P;
    P.chunk_bytes = chunk_bytes > 0 ? chunk_bytes : std::max<int64_t>(n, 16);
    P.unit_max_bytes = unit_max_bytes > 0 ? unit_max_bytes : (int64_t)1 << 27;
    P.guess_mode = guess_mode;
    b.scratch = n + GZ_PAD;
    char err[512] = {0};
    int64_t total = 0;
    const int rc = gz_read(b, n, P, &total, st, err, sizeof(err));
    st[GZ_ST_SCRATCH] = b.scratch;
    if (stats) memcpy(stats, st, sizeof(st));
    if (rc != 0) {
        if (rc != GROM_FASTA_HOST_ONLY) grom_set_last_error(err[0] ? err : "gzip: the read failed");
        return rc;
    }
    uint8_t *o = (uint8_t *)malloc((size_t)total + 1);
    if (!o) return GROM_E_NOMEM;
    memcpy(o, b.text.data(), (size_t)total);
    *out = o;
    *out_len = total;
    return 0;
}

extern "C" void grom_gzip_free(uint8_t *p) { free(p); }
