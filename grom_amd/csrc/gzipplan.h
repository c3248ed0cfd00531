// gzipplan.h -- the host side of the parallel gzip read,
// shared by the device path (gzipdev.hip) and its host twin (gzip_host.cpp):
// member headers and trailers, the chain that takes or refuses the guessed
// units, the output offsets, the groups of the window hand-over and the CRC
// slices joined.  The backend B runs the per-lane pieces of gzipinf.h, on the
// device or in a loop:
//   int  guess(chunk_bytes, mode, std::vector<int64_t> &g)   sorted bit positions
//   int  count(const GzJob *, int64_t n, GzRes *)
//   int  fetch(int64_t off, int n, uint8_t *dst)             compressed bytes
//   int  alloc_text(int64_t total)
//   int  symbolic(const GzJob *, int64_t n, GzRes *)
//   int  resolve(const GzUnit *, int64_t n, int64_t per_group, uint32_t *err)
//   int  crc(const GzSlice *, int64_t n, uint32_t *out)
//   void stage(int k)                                        the stage that begins (times)
// each returning 0 or a GROM_E_* code with B.err set.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/grom_amd.h"
#include "gzipinf.h"

struct GzSlice {
    int64_t off, len;
};

enum { GZ_ST_UNITS = 0, GZ_ST_GUESSED = 1, GZ_ST_AGAIN = 2, GZ_ST_MARKERS = 3, GZ_ST_MEMBERS = 4, GZ_ST_SPAN = 5,
       GZ_ST_SCRATCH = 6, GZ_ST_GROUPS = 7 };
enum { GZ_STAGE_GUESS = 0, GZ_STAGE_COUNT = 1, GZ_STAGE_SYM = 2, GZ_STAGE_HAND = 3, GZ_STAGE_RESOLVE = 4, GZ_STAGE_CRC = 5,
       GZ_STAGE_END = 6 };

#define GZ_CRC_SLICE ((int64_t)65536)

struct GzParams {
    int64_t chunk_bytes = 16384;          // GROM_GZIP_CHUNK_KB
    int64_t unit_max_bytes = 256 << 10;   // GROM_GZIP_UNIT_MAX_KB
    int guess_mode = 1;                   // GROM_GZIP_GUESS
};

// the gzip member header at byte `at` of a file of n bytes: the offset of its
// DEFLATE data, or -1 (not a gzip header, or cut short)
template <class B>
int64_t gz_member_header(B &b, int64_t at, int64_t n) {
    uint8_t h[10];
    if (at + 10 > n || b.fetch(at, 10, h)) return -1;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || (h[3] & 0xe0)) return -1;
    const int flg = h[3];
    int64_t p = at + 10;
    if (flg & 4) {  // FEXTRA
        uint8_t x[2];
        if (p + 2 > n || b.fetch(p, 2, x)) return -1;
        p += 2 + (x[0] | x[1] << 8);
    }
    for (int bit = 8; bit <= 16; bit <<= 1)  // FNAME, FCOMMENT: NUL-terminated
        if (flg & bit) {
            for (;;) {
                uint8_t s[256];
                const int k = (int)std::min<int64_t>(256, n - p);
                if (k <= 0 || b.fetch(p, k, s)) return -1;
                const void *z = memchr(s, 0, (size_t)k);
                if (z) { p += (const uint8_t *)z - s + 1; break; }
                p += k;
            }
        }
    if (flg & 2) p += 2;  // FHCRC
    return p <= n ? p : -1;
}

// The whole read.  On success 0: the text is the backend's, stats filled.
// GROM_FASTA_HOST_ONLY: a unit longer than the cap.  GROM_E_ARG: a malformed
// stream, with the message in err.
template <class B>
int gz_read(B &b, int64_t n, const GzParams &P, int64_t *text_len, int64_t stats[8], char *err, size_t errn) {
    for (int k = 0; k < 8; k++) stats[k] = 0;
    auto fail = [&](const char *fmt, long long a = 0, long long c = 0) {
        snprintf(err, errn, fmt, a, c);
        return (int)GROM_E_ARG;
    };
    const int64_t max_bits = std::min<int64_t>(std::max<int64_t>(P.unit_max_bytes, 64), (int64_t)1 << 27) * 8;
    b.max_bits = max_bits;
    int rc;
    // guesses, and every guessed unit counted
    b.stage(GZ_STAGE_GUESS);
    std::vector<int64_t> g;
    if (P.guess_mode != 0 && (rc = b.guess(std::max<int64_t>(P.chunk_bytes, 16), P.guess_mode, g)) != 0) return rc;
    std::sort(g.begin(), g.end());
    g.erase(std::unique(g.begin(), g.end()), g.end());
    b.stage(GZ_STAGE_COUNT);
    const int64_t ng = (int64_t)g.size();
    std::vector<GzJob> jobs((size_t)ng);
    std::vector<GzRes> res((size_t)ng);
    for (int64_t i = 0; i < ng; i++) {
        GzJob j = {};
        j.start = g[(size_t)i];
        j.stop = i + 1 < ng ? g[(size_t)i + 1] : GZ_NOSTOP;
        jobs[(size_t)i] = j;
    }
    if (ng && (rc = b.count(jobs.data(), ng, res.data())) != 0) return rc;
    // the chain from the first member's first block
    struct Member {
        int64_t text0, text1;
        uint32_t crc, isize;
    };
    std::vector<Member> mem;
    std::vector<GzJob> take;  // the units taken, in order
    int64_t total = 0, at = 0;
    while (at < n) {
        const int64_t data = gz_member_header(b, at, n);
        if (data < 0)
            return mem.empty() ? fail("gzip: no member header at byte %lld", at)
                               : fail("gzip: bytes that are no gzip member follow member %lld at byte %lld",
                                      (long long)mem.size(), at);
        int64_t p = data * 8;
        int fresh = 1;
        const int64_t text0 = total;
        for (;;) {
            const int64_t j = std::lower_bound(g.begin(), g.end(), p) - g.begin();
            GzRes r;
            if (j < ng && g[(size_t)j] == p && res[(size_t)j].status == GI_OK) {
                r = res[(size_t)j];
                stats[GZ_ST_GUESSED]++;
            } else {
                // no guess here (or a unit that must be judged from its true start): decoded from p to the next guess
                GzJob job = {};
                job.start = p;
                const int64_t jn = std::upper_bound(g.begin(), g.end(), p) - g.begin();
                job.stop = jn < ng ? g[(size_t)jn] : GZ_NOSTOP;
                job.fresh = fresh;
                if ((rc = b.count(&job, 1, &r)) != 0) return rc;
                // (the chunk's first unit and a member's first unit start at no guess by construction)
                if (ng) stats[GZ_ST_AGAIN]++;
            }
            if (r.status == GZ_E_LONG) return GROM_FASTA_HOST_ONLY;
            if (r.status != GI_OK)
                return fail("gzip: member %lld does not inflate (DEFLATE error %lld)", (long long)mem.size() + 1, r.status);
            GzJob u = {};
            u.start = p;
            u.stop = r.end_bit;  // (a writing run stops where the counting run did)
            u.out_off = total;
            u.out_len = r.out_len;
            u.fresh = fresh;
            take.push_back(u);
            stats[GZ_ST_SPAN] = std::max<int64_t>(stats[GZ_ST_SPAN], (r.end_bit - p + 7) / 8);
            total += r.out_len;
            p = r.end_bit;
            fresh = 0;
            if (r.final) break;
        }
        const int64_t tr = (p + 7) / 8;
        uint8_t t8[8];
        if (tr + 8 > n || b.fetch(tr, 8, t8)) return fail("gzip: member %lld has no trailer", (long long)mem.size() + 1);
        Member m;
        m.text0 = text0;
        m.text1 = total;
        m.crc = (uint32_t)t8[0] | (uint32_t)t8[1] << 8 | (uint32_t)t8[2] << 16 | (uint32_t)t8[3] << 24;
        m.isize = (uint32_t)t8[4] | (uint32_t)t8[5] << 8 | (uint32_t)t8[6] << 16 | (uint32_t)t8[7] << 24;
        mem.push_back(m);
        at = tr + 8;
    }
    if (mem.empty()) return fail("gzip: an empty file");
    for (size_t k = 0; k < mem.size(); k++)
        if ((uint32_t)(mem[k].text1 - mem[k].text0) != mem[k].isize)
            return fail("gzip: member %lld fails its ISIZE check (the trailer says %lld bytes mod 2^32)", (long long)k + 1,
                        mem[k].isize);
    const int64_t nu = (int64_t)take.size();
    stats[GZ_ST_UNITS] = nu;
    stats[GZ_ST_MEMBERS] = (int64_t)mem.size();
    *text_len = total;
    if ((rc = b.alloc_text(total)) != 0) return rc;
    // the symbols of every unit taken
    b.stage(GZ_STAGE_SYM);
    std::vector<GzRes> sres((size_t)nu);
    if (nu && (rc = b.symbolic(take.data(), nu, sres.data())) != 0) return rc;
    std::vector<GzUnit> units((size_t)nu);
    int64_t mstart = 0;
    for (int64_t i = 0; i < nu; i++) {
        const GzJob &u = take[(size_t)i];
        if (sres[(size_t)i].status != GI_OK)
            return fail("gzip: a unit at bit %lld does not decode a second time (DEFLATE error %lld)", u.start,
                        sres[(size_t)i].status);
        stats[GZ_ST_MARKERS] += sres[(size_t)i].markers;
        if (u.fresh) mstart = u.out_off;
        GzUnit U = {};
        U.off = u.out_off;
        U.len = u.out_len;
        U.avail = (int32_t)std::min<int64_t>(GZ_WIN, u.out_off - mstart);
        units[(size_t)i] = U;
    }
    // hand-over and resolve: groups of about sqrt(units) units
    b.stage(GZ_STAGE_HAND);
    const int64_t per = std::max<int64_t>(1, (int64_t)std::ceil(std::sqrt((double)std::max<int64_t>(nu, 1))));
    stats[GZ_ST_GROUPS] = nu ? (nu + per - 1) / per : 0;
    uint32_t bad = 0;
    if (nu && (rc = b.resolve(units.data(), nu, per, &bad)) != 0) return rc;
    if (bad) return fail("gzip: a distance points before its member's start");
    // per member: the CRC-32 of its text, from fixed slices
    b.stage(GZ_STAGE_CRC);
    std::vector<GzSlice> sl;
    for (const Member &m : mem)
        for (int64_t o = m.text0; o < m.text1; o += GZ_CRC_SLICE) sl.push_back({o, std::min<int64_t>(GZ_CRC_SLICE, m.text1 - o)});
    std::vector<uint32_t> sc(sl.size());
    if (!sl.empty() && (rc = b.crc(sl.data(), (int64_t)sl.size(), sc.data())) != 0) return rc;
    size_t si = 0;
    for (size_t k = 0; k < mem.size(); k++) {
        uLong c = crc32(0L, Z_NULL, 0);
        for (; si < sl.size() && sl[si].off < mem[k].text1; si++) c = crc32_combine(c, sc[si], (z_off_t)sl[si].len);
        if ((uint32_t)c != mem[k].crc)
            return fail("gzip: member %lld fails its CRC-32 check (the text gives %08llx)", (long long)k + 1, (long long)c);
    }
    b.stage(GZ_STAGE_END);
    return 0;
}
