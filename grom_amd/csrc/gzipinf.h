// gzipinf.h -- the per-lane pieces of the parallel read of one plain gzip
// stream, compiled for the device (gzipdev.hip) and for the
// host (gzip_host.cpp, one lane).  The bit reader, the canonical Huffman
// tables, the block-header state machine and the length/distance bases are
// inflate.h's.
//
//   gz_probe     the strict dynamic-block-header test at one bit offset
//   gz_run       blocks decoded from a bit position to the first block end at
//                or past a stop position: counted, or written as 16-bit
//                symbols (a byte, or GZ_MARK | k = byte k of the 32 KB before
//                the unit)
//   gz_group_map / gz_group_windows / gz_group_resolve
//                the window hand-over as a two-level scan over groups of
//                units, and the symbols resolved to bytes
//   gz_crc_slice CRC-32 of a slice of the text (slicing by 4)
//
// Every load is bounded by the buffer's bit count (the compressed copy is
// followed by GZ_PAD zero bytes for the reader's look-ahead), every store by
// the unit's counted length.
#pragma once
#include <stdint.h>

#include "inflate.h"

#define GZ_WIN 32768
#define GZ_MARK 0x8000u
#define GZ_PAD 64
#define GZ_E_LONG 10  // the unit's compressed span exceeds the cap
#define GZ_NOSTOP INT64_MAX

GI_FN uint64_t gz_ld64(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// The strict test of a dynamic block header at bit `bit` of data[0..nbytes)
// (+ GZ_PAD): BTYPE 2, HLIT <= 286, HDIST <= 30, a complete code-length code,
// all HLIT + HDIST lengths decoded with no repeat before the first length and
// no overrun, a length for symbol 256, a complete literal/length code, and a
// distance code that is complete or a single code of length 1.  `tab` holds
// the code-length code alone: GZ_PROBE_DWORDS rows x LANES.
#define GZ_PROBE_DWORDS 5
template <int LANES>
GI_FN bool gz_probe(const uint8_t *data, int64_t nbytes, int64_t bit, uint32_t *tab, int lane) {
    if ((bit >> 3) + 40 > nbytes) return false;  // (a block this close to the end is reached by the chain)
    const uint8_t *p = data + (bit >> 3);
    const int r = (int)(bit & 7);
    const uint64_t w0 = gz_ld64(p) >> r;  // >= 57 bits
    if (((w0 >> 1) & 3u) != 2u) return false;
    const int nlit = (int)((w0 >> 3) & 31u) + 257, ndist = (int)((w0 >> 8) & 31u) + 1, ncl = (int)((w0 >> 13) & 15u) + 4;
    if (nlit > 286 || ndist > 30) return false;
    // the code-length code's lengths: 3 bits each from bit 17
    const uint64_t w1 = gz_ld64(p + 2) >> r;  // bits 16.. of the header
    const uint64_t w2 = gz_ld64(p + 8) >> r;  // bits 64..
    const uint64_t ord_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 |
                            6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t ord_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    uint64_t cl = 0;
    uint32_t kraft = 0;
    for (int k = 0; k < ncl; k++) {
        const int at = 17 + 3 * k;  // header bit of this length
        const uint32_t v = (uint32_t)(at + 3 <= 16 + 56 ? w1 >> (at - 16) : w2 >> (at - 64)) & 7u;
        const int s = (int)((k < 12 ? ord_lo >> (5 * k) : ord_hi >> (5 * (k - 12))) & 31u);
        cl |= (uint64_t)v << (3 * s);
        kraft += v ? 128u >> v : 0u;
    }
    if (kraft != 128u) return false;
    GiHuffCL clh;
    if (gi_build<LANES, 7, false>(clh, tab, lane, 0, 19,
                                  [cl](int i) -> uint32_t { return (uint32_t)(cl >> (3 * i)) & 7u; }))
        return false;
    GiBits b;
    gi_seek(b, p, r + 17 + 3 * ncl);
    uint32_t kl = 0, kd = 0;  // Kraft sums in units of 2^-15
    int n = 0, prev = -1, eob = 0, nd = 0, d1 = 0;
    const int ntot = nlit + ndist;
    const int64_t room = (nbytes - (bit >> 3)) * 8;
    while (n < ntot) {
        gi_refill(b);
        if (gi_used(b) > room) return false;
        const int s = gi_decode<LANES, 7, false>(b, clh, tab, lane, 0);
        if (s < 0) return false;
        int val;
        const int rep = gi_cl_item(b, s, prev, val);
        if (rep < 0 || n + rep > ntot) return false;
        if (val) {
            int rl = nlit - n;
            rl = rl < 0 ? 0 : (rl > rep ? rep : rl);
            kl += (uint32_t)rl << (15 - val);
            kd += (uint32_t)(rep - rl) << (15 - val);
            nd += rep - rl;
            if (rep - rl > 0 && val == 1) d1 = 1;
            if (n <= 256 && 256 < n + rep) eob = 1;
        }
        n += rep;
        prev = val;
    }
    if (!eob || kl != 32768u) return false;
    return kd == 32768u || (nd == 1 && d1);
}

// the first bit of byte `byte` that passes, or -1
template <int LANES>
GI_FN int gz_probe_byte(const uint8_t *data, int64_t nbytes, int64_t byte, uint32_t *tab, int lane) {
    for (int r = 0; r < 8; r++)
        if (gz_probe<LANES>(data, nbytes, byte * 8 + r, tab, lane)) return r;
    return -1;
}

struct GzRes {
    int64_t end_bit;  // where the run stopped: the bit after a block's end
    int64_t out_len;  // bytes the run produces
    int64_t markers;  // symbols written that depend on the window (a writing run)
    int32_t status;   // GI_OK, a GI_E_* code, GZ_E_LONG
    int32_t final;    // it stopped after a BFINAL block
};

struct GzJob {
    int64_t start, stop;  // bit positions; the run ends at the first block end >= stop, or after a BFINAL block
    int64_t out_off;      // a writing run: its first symbol's index
    int64_t out_len;      // a writing run: the symbols it may write (its counted length)
    int32_t fresh;        // the window before it is empty (a member's first unit)
    int32_t pad;
};

// Blocks decoded from job.start.  WRITE: the symbols go to sym[job.out_off ...].
template <int LANES, bool WRITE>
GI_FN void gz_run(const uint8_t *data, int64_t nbytes, const GzJob &job, int64_t max_bits, uint16_t *sym, uint32_t *tab,
                  int lane, GzRes &res) {
    const uint8_t *in = data + (job.start >> 3);
    const int64_t room = nbytes * 8 - (job.start & ~(int64_t)7);  // bits from `in` to the data's end
    GiBits b;
    gi_open(b, in);
    gi_refill(b);
    gi_bits(b, (int)(job.start & 7));
    GiHuff lit = {}, dist = {};
    GiHdr H = {};
    uint32_t bfinal = 0, rem = 0;
    int64_t o = 0, nmark = 0;
    uint16_t *out = WRITE ? sym + job.out_off : nullptr;
    int mode = GI_M_HDR, rc = GI_OK, final = 0;
    int64_t used = 0;
    while (true) {
        gi_refill(b);
        used = gi_used(b);
        if (used > room) { rc = GI_E_INPUT; break; }
        if (used - (job.start & 7) > max_bits) { rc = GZ_E_LONG; break; }
        bool block_end = false;
        if (mode == GI_M_HDR) {
            const int m = gi_header<LANES>(b, lit, dist, H, tab, lane, bfinal, rem);
            if (m < 0) { rc = -m; break; }
            if (m == GI_M_HDR || m == GI_M_DONE) block_end = true;  // an empty stored block
            else if (m == GI_M_STORED && WRITE && o + rem > job.out_len) { rc = GI_E_OVERRUN; break; }
            mode = m == GI_M_DONE ? GI_M_HDR : m;
        } else if (mode == GI_M_P1 || mode == GI_M_P2) {
            const int m = mode == GI_M_P1 ? gi_cl_step<LANES, false>(b, in, lit, dist, H, tab, lane)
                                          : gi_cl_step<LANES, true>(b, in, lit, dist, H, tab, lane);
            if (m < 0) { rc = -m; break; }
            mode = m;
        } else if (mode == GI_M_SYM) {
            const int s = gi_decode<LANES, 15, true>(b, lit, tab, lane, GI_T_LIT);
            if (s < 0 || s > 285) { rc = GI_E_CODE; break; }
            if (s < 256) {
                if (WRITE) {
                    if (o >= job.out_len) { rc = GI_E_OVERRUN; break; }
                    out[o] = (uint16_t)s;
                }
                o++;
            } else if (s == 256) {
                block_end = true;
                mode = GI_M_HDR;
            } else {
                int lb, le;
                gi_len_code(s, lb, le);
                const int64_t len = (int64_t)lb + gi_bits(b, le);
                gi_refill(b);
                const int d = gi_decode<LANES, 15, false>(b, dist, tab, lane, GI_T_DIST);
                if (d < 0 || d > 29) { rc = GI_E_DIST; break; }
                int db, de;
                gi_dist_code(d, db, de);
                const int64_t dd = (int64_t)db + gi_bits(b, de);
                if (dd > o && (job.fresh || dd > o + GZ_WIN)) { rc = GI_E_DIST; break; }
                if (WRITE) {
                    if (o + len > job.out_len) { rc = GI_E_OVERRUN; break; }
                    for (int64_t j = 0; j < len; j++) {
                        const int64_t src = o + j - dd;
                        const uint16_t v = src >= 0 ? out[src] : (uint16_t)(GZ_MARK | (uint32_t)(GZ_WIN + src));
                        nmark += v >> 15;
                        out[o + j] = v;
                    }
                }
                o += len;
            }
        } else {  // GI_M_STORED: byte-aligned, up to 4 bytes from the bit buffer per trip
            const uint32_t m = rem < 4u ? rem : 4u;
            for (uint32_t j = 0; j < m; j++) {
                const uint32_t v = gi_bits(b, 8);
                if (WRITE) out[o] = (uint16_t)v;  // (o + rem <= out_len was checked at the header)
                o++;
            }
            rem -= m;
            if (!rem) {
                block_end = true;
                mode = GI_M_HDR;
            }
        }
        if (block_end) {
            used = gi_used(b);
            if (used > room) { rc = GI_E_INPUT; break; }
            if (bfinal) { final = 1; break; }
            if ((job.start & ~(int64_t)7) + used >= job.stop) break;
        }
    }
    res.end_bit = (job.start & ~(int64_t)7) + used;
    res.out_len = o;
    res.markers = nmark;
    res.status = rc;
    res.final = final;
    if (WRITE && rc == GI_OK && o != job.out_len) res.status = GI_E_SIZE;
}

// ---- the window hand-over and the resolve ----
// A unit taken into the text: its symbols are sym[off, off + len).
struct GzUnit {
    int64_t off, len;
    int32_t avail;  // bytes of its member before it, at most GZ_WIN: a marker k needs GZ_WIN - k <= avail
    int32_t pad;
};

// how the lanes of a group's workgroup (or the host's one lane) take turns
#if defined(__HIPCC__)
#define GZ_MFN __host__ __device__ __forceinline__
#else
#define GZ_MFN inline
#endif
struct GzOneLane {
    GZ_MFN int tid() const { return 0; }
    GZ_MFN int nt() const { return 1; }
    GZ_MFN void sync() const {}
};

#define GZ_E 8  // symbols per lane per tile: one 16-byte load, one 8-byte store

// symbol s through the window w (GZ_WIN cells) before its unit
template <class T>
GI_FN T gz_through(uint16_t s, const T *w) {
    return s < GZ_MARK ? (T)s : w[s & (GZ_WIN - 1)];
}

// cell x of the window after unit U, whose window before it is `cur`: one of
// the unit's last GZ_WIN symbols, or a cell of `cur` carried through (a unit
// shorter than the window).  A copied marker may name any cell of `cur`, so
// the window after the unit is built beside `cur`, never in place.
template <class T>
GI_FN T gz_next_cell(const uint16_t *sym, const GzUnit &U, const T *cur, int x) {
    const int64_t p = U.len - GZ_WIN + x;
    return p >= 0 ? gz_through<T>(sym[U.off + p], cur) : cur[(int64_t)x + U.len];
}

// Group map: the units [u0, u1) composed.  A[x] is then byte x of the window
// after the group as a symbol over the window before it (B: GZ_WIN cells of
// scratch).
template <class Ctx>
GI_FN void gz_group_map(const Ctx &c, const uint16_t *sym, const GzUnit *units, int64_t u0, int64_t u1, uint16_t *A,
                        uint16_t *B) {
    for (int x = c.tid(); x < GZ_WIN; x += c.nt()) A[x] = (uint16_t)(GZ_MARK | (uint32_t)x);
    c.sync();
    uint16_t *cur = A, *nxt = B;
    for (int64_t u = u0; u < u1; u++) {
        const GzUnit U = units[u];
        if (U.len == 0) continue;
        for (int x = c.tid(); x < GZ_WIN; x += c.nt()) nxt[x] = gz_next_cell<uint16_t>(sym, U, cur, x);
        c.sync();
        uint16_t *t = cur;
        cur = nxt;
        nxt = t;
    }
    if (cur != A) {
        for (int x = c.tid(); x < GZ_WIN; x += c.nt()) A[x] = cur[x];
        c.sync();
    }
}

// The window before every group: win[g + 1] = group g's map applied to win[g]
// (win[0] is zeros).  One workgroup.
template <class Ctx>
GI_FN void gz_group_windows(const Ctx &c, const uint16_t *maps, int64_t ngroups, uint8_t *win) {
    for (int x = c.tid(); x < GZ_WIN; x += c.nt()) win[x] = 0;
    c.sync();
    for (int64_t g = 0; g + 1 < ngroups; g++) {
        const uint16_t *m = maps + g * GZ_WIN;
        const uint8_t *w = win + g * GZ_WIN;
        for (int x = c.tid(); x < GZ_WIN; x += c.nt()) win[(g + 1) * GZ_WIN + x] = gz_through<uint8_t>(m[x], w);
        c.sync();
    }
}

// The units [u0, u1) of a group resolved through their windows into
// text[off ...]; W0 and W1 (GZ_WIN bytes each: LDS on the device) hold the
// window before the current unit and the one after it.  A marker that reaches
// before the member's start sets *err.
template <class Ctx>
GI_FN void gz_group_resolve(const Ctx &c, const uint16_t *sym, const GzUnit *units, int64_t u0, int64_t u1,
                            const uint8_t *win, uint8_t *W0, uint8_t *W1, uint8_t *text, uint32_t *err) {
    for (int x = c.tid() * 4; x < GZ_WIN; x += c.nt() * 4) __builtin_memcpy(W0 + x, win + x, 4);
    c.sync();
    uint8_t *cur = W0, *nxt = W1;
    bool bad = false;
    for (int64_t u = u0; u < u1; u++) {
        const GzUnit U = units[u];
        if (U.len == 0) continue;
        const int64_t end = U.off + U.len;
        // tiles of the text, aligned to GZ_E bytes (the lane's store is one aligned 8-byte word)
        for (int64_t t = U.off & ~(int64_t)(GZ_E - 1); t < end; t += (int64_t)c.nt() * GZ_E) {
            const int64_t a = t + (int64_t)c.tid() * GZ_E;
            if (a >= end) continue;
            const bool whole = a >= U.off && a + GZ_E <= end;
            uint16_t s[GZ_E];
            uint8_t v[GZ_E];
            if (whole) __builtin_memcpy(s, sym + a, 2 * GZ_E);
            else
                for (int e = 0; e < GZ_E; e++) s[e] = (a + e >= U.off && a + e < end) ? sym[a + e] : 0;
            for (int e = 0; e < GZ_E; e++) {
                bad = bad || (s[e] >= GZ_MARK && (int32_t)(GZ_WIN - (s[e] & (GZ_WIN - 1))) > U.avail);
                v[e] = gz_through<uint8_t>(s[e], cur);
            }
            if (whole) __builtin_memcpy(text + a, v, GZ_E);
            else
                for (int e = 0; e < GZ_E; e++)
                    if (a + e >= U.off && a + e < end) text[a + e] = v[e];
        }
        if (u + 1 < u1) {
            for (int x = c.tid(); x < GZ_WIN; x += c.nt()) nxt[x] = gz_next_cell<uint8_t>(sym, U, cur, x);
            c.sync();
            uint8_t *t = cur;
            cur = nxt;
            nxt = t;
        }
    }
    if (bad) *err = 1;
}

// ---- CRC-32 (the gzip trailer's), slicing by 4; T is 4 x 256 words ----
GI_FN uint32_t gz_crc_entry(int t, int i, const uint32_t *T) {  // T[0] complete before t > 0
    if (t == 0) {
        uint32_t c = (uint32_t)i;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
        return c;
    }
    const uint32_t p = T[(t - 1) * 256 + i];
    return (p >> 8) ^ T[p & 255u];
}

GI_FN uint32_t gz_crc_slice(const uint8_t *p, int64_t n, const uint32_t *T) {
    uint32_t c = 0xffffffffu;
    while (n > 0 && ((uintptr_t)p & 3)) {
        c = (c >> 8) ^ T[(c ^ *p++) & 255u];
        n--;
    }
    for (; n >= 4; n -= 4, p += 4) {
        uint32_t w;
        __builtin_memcpy(&w, p, 4);
        c ^= w;
        c = T[768 + (c & 255u)] ^ T[512 + ((c >> 8) & 255u)] ^ T[256 + ((c >> 16) & 255u)] ^ T[c >> 24];
    }
    for (; n > 0; n--) c = (c >> 8) ^ T[(c ^ *p++) & 255u];
    return ~c;
}
