// vcfsort.h -- the per-row arithmetic of the sorting, indexing VCF writer
// (DESIGN.md 4.9).  Host/device twin: the kernels of vcfsort.hip run these on
// one lane per row, vcfsort_host.cpp runs them in loops; both must give the
// same facts, keys, offsets and bins, so the three files come out byte for
// byte the same.
//
// A row's facts (VsFacts) come from its first eight columns:
//   CHROM   the bytes before the first tab (compared, never copied)
//   POS     decimal, at least one digit, nothing else
//   REF     its length
//   INFO    the value of the key END (at INFO's start or after ';', followed
//           by '=', decimal)
//   beg0 = max(POS - 1, 0); end0 = beg0 + len(REF); END=v with v > beg0 gives
//   end0 = v; end0 <= beg0 gives end0 = beg0 + 1.
// The .tbi's binning scheme (min shift 14, 5 levels) ends at 2^29.
#pragma once
#include <stdint.h>

#include "inflate.h"  // GI_FN

#define VS_PAYLOAD 65280               // the BGZF writer's uncompressed bytes per block (bgzfdef.h, DF_MAX_PAYLOAD)
#define VS_MAX_END ((int64_t)1 << 29)  // the .tbi limit: 512 Mb
#define VS_NONE 0xffffffffffffffffull  // a linear window without a row

// what is wrong with a line, in the order they are looked for
enum { VS_OK = 0, VS_E_HASH = 1, VS_E_COLS = 2, VS_E_POS = 3, VS_E_LIMIT = 4 };

struct VsFacts {
    uint32_t pos;   // POS as written (saturated at 2^31 - 1)
    int32_t beg0, end0;
    int32_t err;    // VS_OK or VS_E_COLS / VS_E_POS / VS_E_LIMIT
};

// the facts of the row text[a, b), b just past its '\n'
GI_FN VsFacts vs_facts(const uint8_t *text, int64_t a, int64_t b) {
    VsFacts f;
    f.pos = 0, f.beg0 = 0, f.end0 = 1, f.err = VS_OK;
    const int64_t e = b - 1;  // the '\n'
    int64_t p = a;
    while (p < e && text[p] != '\t') p++;  // CHROM
    if (p >= e) { f.err = VS_E_COLS; return f; }
    p++;
    uint64_t v = 0;
    int nd = 0, bad = 0;
    while (p < e && text[p] != '\t') {  // POS
        const uint32_t c = text[p];
        if (c < '0' || c > '9') bad = 1;
        else if (v < 0x7fffffffull) v = v * 10 + (c - '0');
        nd++;
        p++;
    }
    if (v > 0x7fffffffull) v = 0x7fffffffull;
    int64_t ref_len = 0, info = -1;
    int col = 1;
    // ID, REF, ALT, QUAL, FILTER: only REF's length matters
    while (p < e && col < 7) {
        p++;  // the tab
        col++;
        const int64_t s = p;
        if (col == 7) { info = s; break; }
        while (p < e && text[p] != '\t') p++;
        if (col == 3) ref_len = p - s;
    }
    if (info < 0) { f.err = VS_E_COLS; return f; }
    if (bad || nd == 0) { f.err = VS_E_POS; return f; }
    // INFO: the first END= at its start or after ';'
    uint64_t end_v = 0;
    int at_key = 1, found = 0;
    for (p = info; p < e && text[p] != '\t' && !found; p++) {
        if (at_key && p + 3 < e && text[p] == 'E' && text[p + 1] == 'N' && text[p + 2] == 'D' && text[p + 3] == '=') {
            found = 1;
            for (int64_t q = p + 4; q < e && text[q] >= '0' && text[q] <= '9'; q++)
                if (end_v < 0x7fffffffull) end_v = end_v * 10 + (uint32_t)(text[q] - '0');
        }
        at_key = text[p] == ';';
    }
    f.pos = (uint32_t)v;
    const int64_t beg0 = v > 0 ? (int64_t)v - 1 : 0;
    int64_t end0 = beg0 + ref_len;
    if (found && (int64_t)end_v > beg0) end0 = (int64_t)end_v;
    if (end0 <= beg0) end0 = beg0 + 1;
    if (end0 > VS_MAX_END) { f.err = VS_E_LIMIT; return f; }
    f.beg0 = (int32_t)beg0;
    f.end0 = (int32_t)end0;
    return f;
}

// whether the rows at a and b (both end in '\n' before `n`) have the same CHROM bytes
GI_FN bool vs_same_chrom(const uint8_t *text, int64_t a, int64_t b, int64_t n) {
    for (;; a++, b++) {
        const uint32_t x = a < n ? text[a] : '\n', y = b < n ? text[b] : '\n';
        const bool xe = x == '\t' || x == '\n', ye = y == '\t' || y == '\n';
        if (xe || ye) return xe && ye;
        if (x != y) return false;
    }
}

// the UCSC bin of [beg, end), min shift 14, 5 levels (SAM v1 5.3)
GI_FN uint32_t vs_reg2bin(int32_t beg, int32_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// the virtual offset of byte u of the sorted stream of `total` bytes in n_blk
// blocks: coff[0..n_blk) the blocks' file offsets, coff[n_blk] the EOF
// marker's.  The stream's end is the EOF block's start, as a reader that has
// consumed the last block reports it.
GI_FN uint64_t vs_voff(const int64_t *coff, int64_t n_blk, int64_t total, int64_t u) {
    if (u >= total) return (uint64_t)coff[n_blk] << 16;
    return ((uint64_t)coff[u / VS_PAYLOAD] << 16) | (uint64_t)(u % VS_PAYLOAD);
}

// the sort key: the contig id above POS
GI_FN uint64_t vs_key(uint32_t cid, uint32_t pos) { return ((uint64_t)cid << 32) | pos; }
