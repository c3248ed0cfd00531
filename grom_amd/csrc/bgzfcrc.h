// bgzfcrc.h -- the CRC-32 of one inflated BGZF block, striped over the 64
// lanes of a wave.  Host/device twin: k_bgzf_crc
// (ddecode.hip) runs bc_lane on every lane and reduces with shuffles,
// bgzfcrc_host.cpp runs the same stages with the lanes as a loop.
//
// CRC-32 is linear over GF(2).  With R(d) the raw register after the bytes d
// from a zero register (no initial value, no final complement):
//   R(a || b) = R(a) * x^(8 |b|)  ^  R(b)        (mod P, reflected bits)
//   R(0^k || d) = R(d)                            (leading zeros change nothing)
// so a block is cut on a grid of 16-byte chunks at 16-byte-aligned addresses
// (the bytes before its first byte read as zero), lane l takes the chunks
// l, l + 64, ... -- a data step of slicing-by-16, then an advance over the
// 1008 bytes the other lanes own, a multiplication by x^(8*1008) done with a
// 4 x 256 table -- and each lane's value is advanced to the start of the
// block's last chunk (a multiplication by x^(128 g), g <= 63 chunks).  The
// XOR of the lanes is advanced over the last chunk's r = 1..16 bytes and
// takes that chunk's own value; the last chunk is shifted up inside its 16
// bytes so that its data ends where the chunk ends (zeros in front again).
// The all-ones initial register is folded into the data: it equals a zero
// register with the block's first four bytes complemented (for n < 4 the
// register's unused bytes remain: 0xffffffff >> 8n).
//
// Tables, in LDS on the device (BC_DWORDS dwords, 20.9 KB):
//   T[t][i]  byte i followed by t zero bytes, t = 0..15     (16 KB)
//   S[j][i]  (i << 8j) * x^(8*1008)                         (4 KB)
//   X[j]     x^(8 * 2^j), j < 20       (bc_xpow8's square-and-multiply)
//   G[g]     x^(128 g), g < 64;  XR[r] x^(8 r), r <= 16
// Every load of the block stays inside out[0, out_cap).
#pragma once
#include <stdint.h>

#include "inflate.h"

#define BC_POLY 0xedb88320u
#define BC_ONE 0x80000000u  // x^0 (reflected: bit 31 is the constant term)
#define BC_LANES 64
#define BC_CHUNK 16
#define BC_SKIP_BYTES (BC_LANES * BC_CHUNK - BC_CHUNK)  // 1008
#define BC_T 0
#define BC_S (16 * 256)
#define BC_X (BC_S + 4 * 256)
#define BC_NX 20
#define BC_G (BC_X + 32)
#define BC_XR (BC_G + 64)
#define BC_DWORDS (BC_XR + 32)

// a * b mod P
GI_FN uint32_t bc_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        p ^= b & (0u - ((a >> (31 - i)) & 1u));
        b = (b >> 1) ^ (BC_POLY & (0u - (b & 1u)));
    }
    return p;
}

// ---- table entries (every stage reads only the stages before it) ----
GI_FN uint32_t bc_t_entry(int t, int i, const uint32_t *tab) {  // T[0] complete before t > 0, T[t-1] before T[t]
    if (t == 0) {
        uint32_t c = (uint32_t)i;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (BC_POLY & (0u - (c & 1u)));
        return c;
    }
    const uint32_t p = tab[BC_T + (t - 1) * 256 + i];
    return (p >> 8) ^ tab[BC_T + (p & 255u)];
}
GI_FN uint32_t bc_x_entry(int j) {  // x^(8 * 2^j)
    uint32_t v = BC_ONE >> 8;
    for (int k = 0; k < j; k++) v = bc_mulmod(v, v);
    return v;
}
// x^(8 m), m < 2^BC_NX, from X (square-and-multiply)
GI_FN uint32_t bc_xpow8(uint32_t m, const uint32_t *tab) {
    uint32_t p = BC_ONE;
    for (int j = 0; j < BC_NX; j++)
        if ((m >> j) & 1u) p = bc_mulmod(p, tab[BC_X + j]);
    return p;
}
GI_FN uint32_t bc_s_entry(int j, int i, uint32_t xskip) { return bc_mulmod((uint32_t)i << (8 * j), xskip); }

// the table's entries of "thread" t of nt, stage by stage (a barrier between
// the stages): 0..15 T, 16 X, 17 S, G and XR
#define BC_STAGES 18
GI_FN void bc_build_stage(int stage, int t, int nt, uint32_t *tab) {
    if (stage < 16) {
        for (int i = t; i < 256; i += nt) tab[BC_T + stage * 256 + i] = bc_t_entry(stage, i, tab);
    } else if (stage == 16) {
        for (int j = t; j < BC_NX; j += nt) tab[BC_X + j] = bc_x_entry(j);
    } else {
        const uint32_t xskip = bc_xpow8(BC_SKIP_BYTES, tab);
        for (int e = t; e < 1024; e += nt) tab[BC_S + e] = bc_s_entry(e >> 8, e & 255, xskip);
        for (int g = t; g < 64; g += nt) tab[BC_G + g] = bc_xpow8(16u * (uint32_t)g, tab);
        for (int r = t; r <= 16; r += nt) tab[BC_XR + r] = bc_xpow8((uint32_t)r, tab);
    }
}

// ---- the operators ----
// the register advanced over 1008 zero bytes
GI_FN uint32_t bc_skip(uint32_t c, const uint32_t *tab) {
    return tab[BC_S + (c & 255u)] ^ tab[BC_S + 256 + ((c >> 8) & 255u)] ^ tab[BC_S + 512 + ((c >> 16) & 255u)] ^
           tab[BC_S + 768 + (c >> 24)];
}

struct BcChunk {
    uint32_t w0, w1, w2, w3;
};

// 16 data bytes into the register (slicing-by-16: one dependent lookup round)
GI_FN uint32_t bc_step16(uint32_t c, const BcChunk &k, const uint32_t *tab) {
    const uint32_t *T = tab + BC_T;
    c ^= k.w0;
    return T[15 * 256 + (c & 255u)] ^ T[14 * 256 + ((c >> 8) & 255u)] ^ T[13 * 256 + ((c >> 16) & 255u)] ^
           T[12 * 256 + (c >> 24)] ^ T[11 * 256 + (k.w1 & 255u)] ^ T[10 * 256 + ((k.w1 >> 8) & 255u)] ^
           T[9 * 256 + ((k.w1 >> 16) & 255u)] ^ T[8 * 256 + (k.w1 >> 24)] ^ T[7 * 256 + (k.w2 & 255u)] ^
           T[6 * 256 + ((k.w2 >> 8) & 255u)] ^ T[5 * 256 + ((k.w2 >> 16) & 255u)] ^ T[4 * 256 + (k.w2 >> 24)] ^
           T[3 * 256 + (k.w3 & 255u)] ^ T[2 * 256 + ((k.w3 >> 8) & 255u)] ^ T[1 * 256 + ((k.w3 >> 16) & 255u)] ^
           T[(k.w3 >> 24)];
}

// the bytes [lo, hi) of the dword at stream position p, as a mask
GI_FN uint32_t bc_range_mask(int64_t p, int64_t lo, int64_t hi) {
    int64_t a = lo - p, b = hi - p;
    a = a < 0 ? 0 : (a > 4 ? 4 : a);
    b = b < 0 ? 0 : (b > 4 ? 4 : b);
    const uint32_t ma = a >= 4 ? 0xffffffffu : (1u << (8 * (int)a)) - 1u;
    const uint32_t mb = b >= 4 ? 0xffffffffu : (1u << (8 * (int)b)) - 1u;
    return mb & ~ma;
}

// The chunk at out[pos, pos + 16) (pos a multiple of 16, >= 0) of the block
// out[lo, hi): bytes outside the block read as zero, the block's first four
// bytes come complemented (the initial register).  A chunk that reaches past
// out_cap is gathered byte by byte from inside it.
GI_FN BcChunk bc_load(const uint8_t *out, int64_t out_cap, int64_t pos, int64_t lo, int64_t hi) {
    BcChunk k;
    if (pos + BC_CHUNK <= out_cap) {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint4 v = *reinterpret_cast<const uint4 *>(out + pos);  // (out is 16-byte aligned on the device)
        k.w0 = v.x; k.w1 = v.y; k.w2 = v.z; k.w3 = v.w;
#else
        __builtin_memcpy(&k, out + pos, 16);
#endif
    } else {
        uint32_t w[4] = {0, 0, 0, 0};
        GI_UNROLL
        for (int i = 0; i < 16; i++)
            if (pos + i >= lo && pos + i < hi && pos + i < out_cap) w[i >> 2] |= (uint32_t)out[pos + i] << (8 * (i & 3));
        k.w0 = w[0]; k.w1 = w[1]; k.w2 = w[2]; k.w3 = w[3];
    }
    if (pos < lo + 4 || pos + BC_CHUNK > hi) {  // (the block's first chunks and its last)
        const int64_t ie = lo + 4 < hi ? lo + 4 : hi;
        k.w0 = (k.w0 & bc_range_mask(pos, lo, hi)) ^ bc_range_mask(pos, lo, ie);
        k.w1 = (k.w1 & bc_range_mask(pos + 4, lo, hi)) ^ bc_range_mask(pos + 4, lo, ie);
        k.w2 = (k.w2 & bc_range_mask(pos + 8, lo, hi)) ^ bc_range_mask(pos + 8, lo, ie);
        k.w3 = (k.w3 & bc_range_mask(pos + 12, lo, hi)) ^ bc_range_mask(pos + 12, lo, ie);
    }
    return k;
}

// the chunk moved up by e = 0..15 bytes (zeros enter at its front)
GI_FN BcChunk bc_shift_up(BcChunk k, int e) {
    if (e & 4) { k.w3 = k.w2; k.w2 = k.w1; k.w1 = k.w0; k.w0 = 0; }
    if (e & 8) { k.w3 = k.w1; k.w2 = k.w0; k.w1 = 0; k.w0 = 0; }
    const int bs = 8 * (e & 3);
    if (bs) {
        k.w3 = (k.w3 << bs) | (k.w2 >> (32 - bs));
        k.w2 = (k.w2 << bs) | (k.w1 >> (32 - bs));
        k.w1 = (k.w1 << bs) | (k.w0 >> (32 - bs));
        k.w0 <<= bs;
    }
    return k;
}

// the block's chunk grid: a0 its first chunk's position, nfull the chunks
// before the last one, r the last chunk's bytes (1..16), e its free bytes
struct BcGrid {
    int64_t a0;
    int32_t nfull, r, e;
};
GI_FN BcGrid bc_grid(int64_t o, uint32_t n) {  // n > 0
    BcGrid g;
    g.a0 = o & ~(int64_t)15;
    const int64_t end = o + (int64_t)n, a1 = (end + 15) & ~(int64_t)15;
    g.nfull = (int32_t)((a1 - g.a0) / BC_CHUNK) - 1;
    g.e = (int32_t)(a1 - end);
    g.r = BC_CHUNK - g.e;
    return g;
}

// ---- the per-lane partial: lane's chunks, advanced to the start of the last chunk ----
GI_FN uint32_t bc_lane(const uint8_t *out, int64_t out_cap, int64_t o, uint32_t n, int lane, const uint32_t *tab) {
    const BcGrid g = bc_grid(o, n);
    if (lane >= g.nfull) return 0;
    const int64_t end = o + (int64_t)n;
    uint32_t c = 0;
    int32_t q = lane;
    for (;;) {
        c = bc_step16(c, bc_load(out, out_cap, g.a0 + (int64_t)q * BC_CHUNK, o, end), tab);
        if (q + BC_LANES >= g.nfull) break;
        q += BC_LANES;
        c = bc_skip(c, tab);
    }
    return bc_mulmod(c, tab[BC_G + (g.nfull - 1 - q)]);
}

// ---- the combine: the lanes' XOR, the last chunk, the initial register, the complement ----
GI_FN uint32_t bc_combine(uint32_t lanes_xor, const uint8_t *out, int64_t out_cap, int64_t o, uint32_t n,
                          const uint32_t *tab) {
    if (n == 0) return 0;
    const BcGrid g = bc_grid(o, n);
    const BcChunk k = bc_shift_up(bc_load(out, out_cap, g.a0 + (int64_t)g.nfull * BC_CHUNK, o, o + (int64_t)n), g.e);
    uint32_t c = bc_mulmod(lanes_xor, tab[BC_XR + g.r]) ^ bc_step16(0, k, tab);
    if (n < 4) c ^= 0xffffffffu >> (8 * n);
    return ~c;
}
