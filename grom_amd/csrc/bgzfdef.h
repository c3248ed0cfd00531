// bgzfdef.h -- one BGZF block compressed by one wave.
// Host/device twin: k_bgzf_deflate (bgzfwrite.hip) runs the per-lane functions
// below on the 64 lanes of a wave with a barrier between the phases,
// bgzfdef_host.cpp runs the same phases with the lanes as loops.  All the
// arithmetic is here and is integer arithmetic, so the device's bytes are the
// twin's bytes.
//
// A payload of n <= 65280 bytes becomes one complete BGZF block in a slot of
// DF_SLOT bytes: the 18-byte header (BC subfield, BSIZE), one final DEFLATE
// block, then CRC-32 and ISIZE (df_trailer; the CRC is bgzfcrc.h's).
//
// The parse.  The payload is walked in steps of 64 positions.  In a step
//   1. lane l looks position p = base + l up in a hash table of the latest
//      position of each 4-byte hash (entries from earlier steps only), and
//      measures the match there: length 3..258, distance <= 32768, the source
//      inside this payload;
//   2. after a barrier every lane enters its position with an atomic max, so
//      the bucket's winner is the highest position, whatever the store order;
//   3. lane 0 walks the step's 64 (length, distance) pairs greedily from where
//      the last match ended, one look ahead (a longer match at p + 1 turns p
//      into a literal), appends tokens and counts their symbols.
// A byte histogram is counted on the side (atomic adds commute).
//
// The choice.  Lane 0 builds length-limited Huffman codes (df_build_lengths:
// Moffat-Katajainen minimum-redundancy lengths in place, then the overflow
// moved down level by level until the Kraft sum is 1) and prices four
// candidates exactly: stored, fixed Huffman over the tokens, dynamic Huffman
// over the tokens, dynamic Huffman over the payload as literals only (from the
// byte histogram; a short far match costs ACGT text more than its literals).
// The smallest goes out, ties to the earlier one in that order, so a block
// never exceeds n + 31 bytes.  The dynamic header writes the code lengths
// plainly (no run-length symbols 16/17/18).
//
// The bits.  Lane l takes token t0 + l, a prefix sum of the tokens' bit
// counts places it, and its bits are OR-ed into the zeroed slot (OR commutes).
#pragma once
#include <stdint.h>

#include "inflate.h"

#define DF_MAX_PAYLOAD 65280
#define DF_LANES 64
#define DF_HASH_BITS 13
#define DF_HASH_SIZE (1 << DF_HASH_BITS)
#define DF_MAX_MATCH 258
#define DF_WINDOW 32768
#define DF_NEAR 4096          // a 3-byte match further away than this costs more than its literals
#define DF_SLOT 65344         // >= 65280 + 31, + 16 for the gather's whole-word loads, a multiple of 64
#define DF_TOK_MATCH 0x80000000u
#define DF_NL 288
#define DF_ND 32

enum { DF_STORED = 0, DF_FIXED = 1, DF_DYN = 2, DF_LITDYN = 3 };

#if defined(__HIP_DEVICE_COMPILE__)
#define DF_ATOMIC_MAX(p, v) atomicMax((p), (v))
#define DF_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#define DF_ATOMIC_OR(p, v) atomicOr((p), (v))
#else
#define DF_ATOMIC_MAX(p, v) (void)(*(p) = *(p) > (v) ? *(p) : (v))
#define DF_ATOMIC_ADD(p, v) (void)(*(p) += (v))
#define DF_ATOMIC_OR(p, v) (void)(*(p) |= (v))
#endif

// one set of codes: literal/length, distance, and the code-length code of a dynamic header
struct DfCode {
    uint16_t lcode[DF_NL], dcode[DF_ND], clcode[19];
    uint8_t llen[DF_NL], dlen[DF_ND], cllen[19];
    int32_t hlit, hdist, hclen;
    uint32_t hdr_bits, body_bits;  // the dynamic header after the 3 block bits; the symbols, their extra bits and end-of-block
};

// the wave's state (LDS on the device)
struct DfShared {
    uint32_t head[DF_HASH_SIZE];       // position + 1 of the latest entry, 0: none
    uint32_t lfreq[DF_NL], dfreq[DF_ND];  // the tokens' symbols
    uint32_t bfreq[DF_NL];             // the payload's bytes (and one end-of-block)
    uint32_t work[2 * DF_NL];          // the code-length builder's
    uint16_t mlen[DF_LANES + 1], mdist[DF_LANES + 1];
    DfCode code[2];                    // [0] the tokens' code (dynamic, or fixed), [1] the literal-only code
    uint32_t ntok, carry, xbits;       // tokens, where the last match ended, the tokens' extra bits
    int32_t kind;
    uint32_t body_bit, cbytes;         // the chosen block: where its symbols start (a bit offset in the slot), its DEFLATE bytes
};

// ---- the alphabets ----
GI_FN int df_log2(uint32_t v) {  // v > 0
    int r = 0;
    while (v >>= 1) r++;
    return r;
}
GI_FN void df_len_sym(uint32_t l, uint32_t &sym, uint32_t &eb, uint32_t &ev) {  // l = 3..258
    const uint32_t m = l - 3;
    if (l == 258) { sym = 285; eb = 0; ev = 0; return; }
    if (m < 8) { sym = 257 + m; eb = 0; ev = 0; return; }
    eb = (uint32_t)df_log2(m) - 2;
    sym = 261 + 4 * eb + ((m >> eb) & 3u);
    ev = m & ((1u << eb) - 1u);
}
GI_FN void df_dist_sym(uint32_t d, uint32_t &sym, uint32_t &eb, uint32_t &ev) {  // d = 1..32768
    const uint32_t m = d - 1;
    if (m < 4) { sym = m; eb = 0; ev = 0; return; }
    eb = (uint32_t)df_log2(m) - 1;
    sym = 2 * eb + 2 + ((m >> eb) & 1u);
    ev = m & ((1u << eb) - 1u);
}
GI_FN uint32_t df_len_extra(uint32_t sym) { return sym < 265 || sym >= 285 ? 0 : (sym - 261) >> 2; }
GI_FN uint32_t df_dist_extra(uint32_t sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }
GI_FN uint32_t df_cl_order(int i) {
    // RFC 1951 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    if (i < 3) return 16u + (uint32_t)i;
    if (i == 3) return 0;
    const int k = i - 4;  // 8 7 9 6 10 5 ...
    return (k & 1) ? (uint32_t)(7 - (k >> 1)) : (uint32_t)(8 + (k >> 1));
}

// ---- length-limited code lengths ----
// freq[0..n) -> len[0..n), every length <= limit, Kraft sum exactly 1 when two
// or more symbols are used.  One used symbol gets one bit; with force_two a
// second symbol (0, or 1 when 0 is the used one) is given a code too, as
// zlib does, so that the code is complete.  work: 2 n dwords.  n <= 288.
GI_FN void df_build_lengths(const uint32_t *freq, int n, int limit, int force_two, uint8_t *len, uint32_t *work) {
    uint32_t *key = work, *A = work + n;
    int m = 0;
    for (int i = 0; i < n; i++) {
        len[i] = 0;
        if (freq[i]) key[m++] = (freq[i] << 9) | (uint32_t)i;  // (freq <= 65281: 17 bits)
    }
    if (m == 0) {
        if (!force_two) return;
        key[m++] = (1u << 9) | 0u;
    }
    if (m == 1) {
        if (!force_two) { len[key[0] & 511u] = 1; return; }
        const uint32_t other = (key[0] & 511u) == 0 ? 1u : 0u;
        key[m++] = (1u << 9) | other;
    }
    // ascending by (frequency, symbol): insertion sort
    for (int i = 1; i < m; i++) {
        const uint32_t k = key[i];
        int j = i - 1;
        while (j >= 0 && key[j] > k) { key[j + 1] = key[j]; j--; }
        key[j + 1] = k;
    }
    for (int i = 0; i < m; i++) A[i] = key[i] >> 9;
    // minimum-redundancy code lengths in place (Moffat and Katajainen 1995)
    if (m == 2) {
        A[0] = A[1] = 1;
    } else {
        A[0] += A[1];
        int root = 0, leaf = 2, next;
        for (next = 1; next < m - 1; next++) {
            if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; }
            else A[next] = A[leaf++];
            if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; }
            else A[next] += A[leaf++];
        }
        A[m - 2] = 0;
        for (next = m - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
        int avbl = 1, used = 0, dpth = 0;
        root = m - 2;
        next = m - 1;
        while (avbl > 0) {
            while (root >= 0 && (int)A[root] == dpth) { used++; root--; }
            while (avbl > used) { A[next--] = (uint32_t)dpth; avbl--; }
            avbl = 2 * used;
            dpth++;
            used = 0;
        }
    }
    // A[i]: the length of the i-th rarest symbol, non-increasing.  Limit them.
    uint32_t cnt[40];
    for (int i = 0; i < 40; i++) cnt[i] = 0;
    bool over = false;
    for (int i = 0; i < m; i++) {
        uint32_t l = A[i];
        if (l > (uint32_t)limit) { l = (uint32_t)limit; over = true; }
        cnt[l]++;
    }
    if (over) {
        uint32_t total = 0;  // the Kraft sum in units of 2^-limit
        for (int l = 1; l <= limit; l++) total += cnt[l] << (limit - l);
        while (total > (1u << limit)) {
            // one code of the limit's length leaves, one shorter code is split in two
            cnt[limit]--;
            for (int l = limit - 1; l >= 1; l--)
                if (cnt[l]) { cnt[l]--; cnt[l + 1] += 2; break; }
            total--;
        }
    }
    // the rarest symbols take the longest codes
    int i = 0;
    for (int l = limit; l >= 1; l--)
        for (uint32_t c = cnt[l]; c > 0; c--) len[key[i++] & 511u] = (uint8_t)l;
}

// canonical codes, bit-reversed for the LSB-first stream
GI_FN void df_assign_codes(const uint8_t *len, int n, uint16_t *code) {
    uint32_t cnt[16], nxt[16];
    for (int l = 0; l < 16; l++) cnt[l] = 0;
    for (int i = 0; i < n; i++) cnt[len[i]]++;
    cnt[0] = 0;
    uint32_t c = 0;
    nxt[0] = 0;
    for (int l = 1; l < 16; l++) { c = (c + cnt[l - 1]) << 1; nxt[l] = c; }
    for (int i = 0; i < n; i++) {
        const int l = len[i];
        uint32_t v = 0;
        if (l) {
            const uint32_t x = nxt[l]++;
            for (int b = 0; b < l; b++) v |= ((x >> b) & 1u) << (l - 1 - b);
        }
        code[i] = (uint16_t)v;
    }
}

// ---- bits into the zeroed slot ----
GI_FN void df_put(uint32_t *out, uint32_t bitpos, uint32_t v, uint32_t nb) {  // nb <= 32, v < 2^nb
    if (nb == 0 || (bitpos >> 5) + 1 >= DF_SLOT / 4) return;  // (never past the slot, whatever the caller computed)
    const uint64_t w = (uint64_t)v << (bitpos & 31u);
    const uint32_t lo = (uint32_t)w, hi = (uint32_t)(w >> 32);
    if (lo) DF_ATOMIC_OR(out + (bitpos >> 5), lo);
    if (hi) DF_ATOMIC_OR(out + (bitpos >> 5) + 1, hi);
}

// ---- the phases ----
GI_FN void df_init(DfShared *S, int lane) {
    for (int i = lane; i < DF_HASH_SIZE; i += DF_LANES) S->head[i] = 0;
    for (int i = lane; i < DF_NL; i += DF_LANES) { S->lfreq[i] = 0; S->bfreq[i] = 0; }
    for (int i = lane; i < DF_ND; i += DF_LANES) S->dfreq[i] = 0;
    if (lane == 0) { S->ntok = 0; S->carry = 0; S->xbits = 0; S->kind = 0; }
}

GI_FN uint32_t df_hash(const uint8_t *p) {
    const uint32_t w = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    return (w * 2654435761u) >> (32 - DF_HASH_BITS);
}

// phase 1: the match at base + lane (reads head, writes mlen / mdist)
GI_FN void df_match(DfShared *S, const uint8_t *in, uint32_t n, uint32_t base, int lane) {
    const uint32_t p = base + (uint32_t)lane;
    uint32_t ml = 0, md = 0;
    if (p < n) DF_ATOMIC_ADD(&S->bfreq[in[p]], 1u);
    // (a position inside the last match is never asked for, nor the one before a step's first)
    if (p + 4 <= n && p >= S->carry) {
        const uint32_t c = S->head[df_hash(in + p)];
        if (c != 0 && p - (c - 1) <= DF_WINDOW) {
            const uint32_t q = c - 1, lim = n - p < DF_MAX_MATCH ? n - p : DF_MAX_MATCH;
            uint32_t l = 0;
            while (l < lim && in[q + l] == in[p + l]) l++;
            if (l >= 4 || (l == 3 && p - q <= DF_NEAR)) { ml = l; md = p - q; }
        }
    }
    S->mlen[lane] = (uint16_t)ml;
    S->mdist[lane] = (uint16_t)(md - (md ? 1u : 0u));
}

// phase 2: base + lane entered (the highest position of a bucket wins)
GI_FN void df_insert(DfShared *S, const uint8_t *in, uint32_t n, uint32_t base, int lane) {
    const uint32_t p = base + (uint32_t)lane;
    if (p + 4 <= n) DF_ATOMIC_MAX(&S->head[df_hash(in + p)], p + 1);
}

// phase 3 (lane 0): the step's tokens
GI_FN void df_parse(DfShared *S, const uint8_t *in, uint32_t n, uint32_t base, uint32_t *tok) {
    const uint32_t end = base + DF_LANES < n ? base + DF_LANES : n;
    uint32_t pos = S->carry, nt = S->ntok, xb = S->xbits;
    while (pos < end) {
        const uint32_t i = pos - base;
        uint32_t l = S->mlen[i];
        if (l && pos + 1 < end && S->mlen[i + 1] > l + 1) l = 0;  // the next position's match is longer
        if (l) {
            uint32_t ls, le, lv, ds, de, dv;
            const uint32_t d = (uint32_t)S->mdist[i] + 1;
            df_len_sym(l, ls, le, lv);
            df_dist_sym(d, ds, de, dv);
            S->lfreq[ls]++;
            S->dfreq[ds]++;
            xb += le + de;
            tok[nt++] = DF_TOK_MATCH | (l - 3) << 16 | (d - 1);
            pos += l;
        } else {
            S->lfreq[in[pos]]++;
            tok[nt++] = in[pos];
            pos++;
        }
    }
    S->carry = pos;
    S->ntok = nt;
    S->xbits = xb;
}

// the dynamic header of a code whose llen / dlen are set: hlit, hdist, the
// code-length code, hdr_bits
GI_FN void df_dyn_header(DfCode *C, uint32_t *work) {
    int hlit = 286, hdist = 30;
    while (hlit > 257 && C->llen[hlit - 1] == 0) hlit--;
    while (hdist > 1 && C->dlen[hdist - 1] == 0) hdist--;
    uint32_t clf[19];
    for (int i = 0; i < 19; i++) clf[i] = 0;
    for (int i = 0; i < hlit; i++) clf[C->llen[i]]++;
    for (int i = 0; i < hdist; i++) clf[C->dlen[i]]++;
    df_build_lengths(clf, 19, 7, 1, C->cllen, work);
    df_assign_codes(C->cllen, 19, C->clcode);
    int hclen = 19;
    while (hclen > 4 && C->cllen[df_cl_order(hclen - 1)] == 0) hclen--;
    uint32_t bits = 5 + 5 + 4 + 3 * (uint32_t)hclen;
    for (int i = 0; i < 19; i++) bits += clf[i] * C->cllen[i];
    C->hlit = hlit;
    C->hdist = hdist;
    C->hclen = hclen;
    C->hdr_bits = bits;
}

GI_FN void df_fixed_code(DfCode *C) {
    for (int i = 0; i < DF_NL; i++) C->llen[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    for (int i = 0; i < DF_ND; i++) C->dlen[i] = 5;
    df_assign_codes(C->llen, DF_NL, C->lcode);
    df_assign_codes(C->dlen, DF_ND, C->dcode);
}

// after the last step (lane 0): the four candidates priced, the smallest's
// BGZF header and block header written.  Sets kind, body_bit, cbytes.
GI_FN void df_plan(DfShared *S, uint32_t n, uint32_t *out) {
    S->lfreq[256] = 1;
    S->bfreq[256] = 1;
    DfCode *T = &S->code[0], *L = &S->code[1];
    // dynamic over the tokens
    df_build_lengths(S->lfreq, 286, 15, 1, T->llen, S->work);
    df_build_lengths(S->dfreq, 30, 15, 0, T->dlen, S->work);
    for (int i = 286; i < DF_NL; i++) T->llen[i] = 0;
    for (int i = 30; i < DF_ND; i++) T->dlen[i] = 0;
    df_dyn_header(T, S->work);
    uint32_t body = S->xbits, fixed = S->xbits;
    for (int i = 0; i < 286; i++) {
        body += S->lfreq[i] * T->llen[i];
        fixed += S->lfreq[i] * (uint32_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    }
    for (int i = 0; i < 30; i++) {
        body += S->dfreq[i] * T->dlen[i];
        fixed += S->dfreq[i] * 5u;
    }
    T->body_bits = body;
    // dynamic over the payload as literals
    df_build_lengths(S->bfreq, 286, 15, 1, L->llen, S->work);
    for (int i = 286; i < DF_NL; i++) L->llen[i] = 0;
    for (int i = 0; i < DF_ND; i++) L->dlen[i] = 0;
    df_dyn_header(L, S->work);
    body = 0;
    for (int i = 0; i <= 256; i++) body += S->bfreq[i] * L->llen[i];
    L->body_bits = body;
    const uint32_t cost[4] = {5 + n, (3 + fixed + 7) >> 3, (3 + T->hdr_bits + T->body_bits + 7) >> 3,
                              (3 + L->hdr_bits + L->body_bits + 7) >> 3};
    int kind = 0;
    for (int k = 1; k < 4; k++)
        if (cost[k] < cost[kind]) kind = k;
    S->kind = kind;
    S->cbytes = cost[kind];
    // the BGZF header: 1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C' 2 0, BSIZE = size - 1
    const uint32_t bsize = 18 + S->cbytes + 8 - 1;
    out[0] = 0x04088b1fu;
    out[1] = 0;
    out[2] = 0x0006ff00u;
    out[3] = 0x00024342u;
    out[4] = bsize;  // (bytes 16 and 17; the DEFLATE data follows at bit 144)
    uint32_t bp = 144;
    if (kind == DF_STORED) {
        df_put(out, bp, 1, 8);  // BFINAL 1, BTYPE 00, to the byte's end
        df_put(out, bp + 8, n, 16);
        df_put(out, bp + 24, ~n & 0xffffu, 16);
        S->body_bit = bp + 40;
        return;
    }
    if (kind == DF_FIXED) {
        df_put(out, bp, 3, 3);  // BFINAL 1, BTYPE 01
        df_fixed_code(T);
        S->body_bit = bp + 3;
        return;
    }
    DfCode *C = kind == DF_DYN ? T : L;
    df_assign_codes(C->llen, DF_NL, C->lcode);
    df_assign_codes(C->dlen, DF_ND, C->dcode);
    df_put(out, bp, 5, 3);  // BFINAL 1, BTYPE 10
    bp += 3;
    df_put(out, bp, (uint32_t)(C->hlit - 257), 5);
    df_put(out, bp + 5, (uint32_t)(C->hdist - 1), 5);
    df_put(out, bp + 10, (uint32_t)(C->hclen - 4), 4);
    bp += 14;
    for (int i = 0; i < C->hclen; i++, bp += 3) df_put(out, bp, C->cllen[df_cl_order(i)], 3);
    for (int i = 0; i < C->hlit; i++) {
        df_put(out, bp, C->clcode[C->llen[i]], C->cllen[C->llen[i]]);
        bp += C->cllen[C->llen[i]];
    }
    for (int i = 0; i < C->hdist; i++) {
        df_put(out, bp, C->clcode[C->dlen[i]], C->cllen[C->dlen[i]]);
        bp += C->cllen[C->dlen[i]];
    }
    S->body_bit = bp;
}

// one token's bits under code C: the literal or length part (<= 20 bits) and the distance part (<= 28)
GI_FN void df_token_bits(const DfCode *C, uint32_t t, uint32_t &v0, uint32_t &n0, uint32_t &v1, uint32_t &n1) {
    if (!(t & DF_TOK_MATCH)) {
        v0 = C->lcode[t & 255u];
        n0 = C->llen[t & 255u];
        v1 = 0;
        n1 = 0;
        return;
    }
    uint32_t ls, le, lv, ds, de, dv;
    df_len_sym(((t >> 16) & 255u) + 3, ls, le, lv);
    df_dist_sym((t & 0x7fffu) + 1, ds, de, dv);
    v0 = (uint32_t)C->lcode[ls] | lv << C->llen[ls];
    n0 = C->llen[ls] + le;
    v1 = (uint32_t)C->dcode[ds] | dv << C->dlen[ds];
    n1 = C->dlen[ds] + de;
}

// the trailer, once the payload's CRC-32 is known
GI_FN void df_trailer(uint8_t *slot, uint32_t size, uint32_t crc, uint32_t n) {
    uint8_t *t = slot + size - 8;
    for (int k = 0; k < 4; k++) {
        t[k] = (uint8_t)(crc >> (8 * k));
        t[4 + k] = (uint8_t)(n >> (8 * k));
    }
}
