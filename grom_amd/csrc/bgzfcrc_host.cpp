// bgzfcrc_host.cpp -- the host side of the BGZF checksum work (DESIGN.md
// 4.5, item 9): the host twin of k_bgzf_crc (bgzfcrc.h's stages with the 64 lanes as
// a loop; tests/test_bgzf_crc_host.py and tools/crc_check.cpp compare it with
// zlib), and grom_bgzf_check, the one-thread file check on zlib's inflate and
// crc32 that the device check is compared with.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <chrono>
#include <mutex>
#include <vector>

#include "../../include/grom_amd.h"
#include "bgzfcrc.h"

namespace {

uint32_t g_tab[BC_DWORDS];
std::once_flag g_tab_once;

// the kernel's table build: 256 "threads", a barrier between the stages
void build_tab() {
    for (int s = 0; s < BC_STAGES; s++)
        for (int t = 0; t < 256; t++) bc_build_stage(s, t, 256, g_tab);
}

uint16_t rd16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
uint32_t rd32(const uint8_t *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

const uint8_t EOF_BLOCK[28] = {0x1f, 0x8b, 0x08, 0x04, 0x00, 0x00, 0x00, 0x00, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43,
                               0x02, 0x00, 0x1b, 0x00, 0x03, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00};

}  // namespace

extern "C" uint32_t grom_bgzf_crc_twin(const uint8_t *buf, int64_t cap, int64_t off, uint32_t n) {
    std::call_once(g_tab_once, build_tab);
    if (off < 0 || off + (int64_t)n > cap) return 0;
    uint32_t v = 0;
    for (int lane = 0; lane < BC_LANES; lane++) v ^= bc_lane(buf, cap, off, n, lane, g_tab);
    return bc_combine(v, buf, cap, off, n, g_tab);
}

extern "C" int grom_bgzf_check(const char *path, int64_t out[8], int64_t *bad_off, int64_t bad_cap) {
    const auto t0 = std::chrono::steady_clock::now();
    if (out) memset(out, 0, 8 * sizeof(int64_t));
    char msg[4400];
    FILE *fp = path ? fopen(path, "rb") : nullptr;
    if (!fp) {
        snprintf(msg, sizeof(msg), "BGZF check: cannot open %s", path ? path : "(no path)");
        grom_set_last_error(msg);
        return GROM_E_ARG;
    }
    int64_t n_blk = 0, n_bad = 0, first = -1, ubytes = 0, off = 0;
    int eof_marker = 0, rc = 0;
    std::vector<uint8_t> cb(65536 + 64), ub(65536 + 64);
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, -15) != Z_OK) {
        fclose(fp);
        grom_set_last_error("BGZF check: out of memory");
        return GROM_E_NOMEM;
    }
    for (;;) {
        const size_t got = fread(cb.data(), 1, 18, fp);
        if (got == 0) break;
        bool whole = got == 18 && cb[0] == 0x1f && cb[1] == 0x8b && cb[2] == 8 && (cb[3] & 4);
        int xlen = 0, bsize = -1;
        if (whole) {
            xlen = rd16(cb.data() + 10);
            whole = xlen >= 6 && (xlen == 6 || fread(cb.data() + 18, 1, (size_t)xlen - 6, fp) == (size_t)xlen - 6);
        }
        if (whole) {
            for (int o = 0; o + 4 <= xlen;) {
                const int sl = rd16(cb.data() + 12 + o + 2);
                if (cb[12 + o] == 'B' && cb[12 + o + 1] == 'C' && sl == 2) bsize = rd16(cb.data() + 12 + o + 4);
                o += 4 + sl;
            }
            const int64_t blen = (int64_t)bsize + 1, rest = blen - 12 - xlen;
            whole = bsize >= 0 && rest >= 8 && fread(cb.data() + 12 + xlen, 1, (size_t)rest, fp) == (size_t)rest &&
                    rd32(cb.data() + blen - 4) <= 65536;
        }
        if (!whole) {
            snprintf(msg, sizeof(msg), "BGZF check: no whole BGZF block at byte %lld", (long long)off);
            grom_set_last_error(msg);
            rc = GROM_E_ARG;
            break;
        }
        const int64_t blen = (int64_t)bsize + 1;
        const uint32_t isize = rd32(cb.data() + blen - 4), want = rd32(cb.data() + blen - 8);
        bool ok = inflateReset(&zs) == Z_OK;
        if (ok) {
            zs.next_in = cb.data() + 12 + xlen;
            zs.avail_in = (uInt)(blen - 12 - xlen - 8);
            zs.next_out = ub.data();
            zs.avail_out = 65536;
            ok = inflate(&zs, Z_FINISH) == Z_STREAM_END && zs.total_out == isize;
        }
        if (ok) ok = (uint32_t)crc32(crc32(0L, Z_NULL, 0), ub.data(), isize) == want;
        if (!ok) {
            if (first < 0) first = off;
            if (bad_off && n_bad < bad_cap) bad_off[n_bad] = off;
            n_bad++;
        }
        eof_marker = blen == 28 && memcmp(cb.data(), EOF_BLOCK, 28) == 0;
        n_blk++;
        ubytes += isize;
        off += blen;
    }
    inflateEnd(&zs);
    fclose(fp);
    if (out) {
        out[0] = n_blk;
        out[1] = n_bad;
        out[2] = first;
        out[3] = ubytes;
        out[4] = n_blk > 0 ? 1 : 0;
        out[5] = eof_marker;
        out[6] = 0;
        out[7] = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    }
    if (rc == 0 && n_bad > 0) {
        // (a block that did not inflate is named by the same sentence: its bytes cannot have the trailer's CRC)
        snprintf(msg, sizeof(msg), "BGZF block at file offset %lld of %s: CRC-32 mismatch", (long long)first, path);
        grom_set_last_error(msg);
        rc = GROM_E_ARG;
    }
    return rc;
}
