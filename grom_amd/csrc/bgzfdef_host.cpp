// bgzfdef_host.cpp -- the host twin of k_bgzf_deflate:
// bgzfdef.h's phases with the 64 lanes as loops and the barriers as the loops'
// ends, the trailer's CRC-32 from the checksum kernel's twin.  Plain C++, no
// HIP.  tests/test_bgzf_write_host.py and tools/deflate_check.cpp compare its
// blocks with zlib's decoder; the GPU tests demand its bytes from the kernel.
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../include/grom_amd.h"
#include "bgzfdef.h"
#include "bgzfwrite.h"

namespace {

// one payload into the zeroed, 4-byte-aligned slot; its size, or 0 when the bits emitted are not the bits priced
uint32_t twin_block(const uint8_t *in, uint32_t n, uint32_t *out, uint32_t *tok, DfShared *S, int *kind) {
    for (int lane = 0; lane < DF_LANES; lane++) df_init(S, lane);
    for (uint32_t base = 0; base < n; base += DF_LANES) {
        for (int lane = 0; lane < DF_LANES; lane++) df_match(S, in, n, base, lane);
        for (int lane = 0; lane < DF_LANES; lane++) df_insert(S, in, n, base, lane);
        df_parse(S, in, n, base, tok);
    }
    df_plan(S, n, out);
    *kind = S->kind;
    const uint32_t size = 18 + S->cbytes + 8;
    uint8_t *out8 = reinterpret_cast<uint8_t *>(out);
    if (S->kind == DF_STORED) {
        for (int lane = 0; lane < DF_LANES; lane++)
            for (uint32_t i = (uint32_t)lane; i < n; i += DF_LANES) out8[(S->body_bit >> 3) + i] = in[i];
    } else {
        const DfCode *C = &S->code[S->kind == DF_LITDYN ? 1 : 0];
        const uint32_t nt = S->kind == DF_LITDYN ? n : S->ntok;
        uint32_t bp = S->body_bit;
        for (uint32_t t0 = 0; t0 < nt; t0 += DF_LANES) {
            uint32_t at[DF_LANES + 1];
            at[0] = bp;
            for (int lane = 0; lane < DF_LANES; lane++) {  // (the wave's prefix sum)
                uint32_t v0, n0, v1, n1, nb = 0;
                if (t0 + lane < nt) {
                    df_token_bits(C, S->kind == DF_LITDYN ? in[t0 + lane] : tok[t0 + lane], v0, n0, v1, n1);
                    nb = n0 + n1;
                }
                at[lane + 1] = at[lane] + nb;
            }
            for (int lane = 0; lane < DF_LANES; lane++) {
                if (t0 + lane >= nt) break;
                uint32_t v0, n0, v1, n1;
                df_token_bits(C, S->kind == DF_LITDYN ? in[t0 + lane] : tok[t0 + lane], v0, n0, v1, n1);
                df_put(out, at[lane], v0, n0);
                df_put(out, at[lane] + n0, v1, n1);
            }
            bp = at[DF_LANES];
        }
        df_put(out, bp, C->lcode[256], C->llen[256]);
        bp += C->llen[256];
        if (((bp - 144 + 7) >> 3) != S->cbytes) return 0;
    }
    df_trailer(out8, size, n ? grom_bgzf_crc_twin(in, (int64_t)n, 0, n) : 0u, n);
    return size;
}

}  // namespace

extern "C" int df_host_blocks(const uint8_t *buf, const int64_t *offs, int64_t n_blk, uint8_t *dst, int64_t dst_cap,
                              int64_t *dst_offs, int64_t kinds[4]) {
    std::unique_ptr<DfShared> S(new DfShared);
    std::vector<uint32_t> slot(DF_SLOT / 4), tok(DF_MAX_PAYLOAD);
    int64_t o = 0;
    for (int64_t j = 0; j < n_blk; j++) {
        const int64_t n = offs[j + 1] - offs[j];
        if (n < 0 || n > DF_MAX_PAYLOAD) return -1;
        memset(slot.data(), 0, DF_SLOT);
        int kind = 0;
        const uint32_t size = twin_block(buf + offs[j], (uint32_t)n, slot.data(), tok.data(), S.get(), &kind);
        if (size == 0) return -3;
        if (o + (int64_t)size > dst_cap) return -2;
        memcpy(dst + o, slot.data(), size);
        if (dst_offs) dst_offs[j] = o;
        if (kinds) kinds[kind]++;
        o += size;
    }
    if (dst_offs) dst_offs[n_blk] = o;
    return 0;
}

extern "C" void df_host_lengths(const uint32_t *freq, int n, int limit, int force_two, uint8_t *len) {
    std::vector<uint32_t> work(2 * DF_NL);
    df_build_lengths(freq, n, limit, force_two, len, work.data());
}
