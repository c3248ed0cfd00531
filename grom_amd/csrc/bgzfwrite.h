/* bgzfwrite.h -- the BGZF writer's host twin as the rest of the library and
 * the sanitizer program (tools/deflate_check.cpp) call it: bgzfdef.h's phases
 * with the lanes as loops (bgzfdef_host.cpp; no HIP). */
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* n_blk payloads buf[offs[i], offs[i + 1]), each at most 65280 bytes, as
 * concatenated BGZF blocks in dst[0, dst_cap): dst_offs[0..n_blk] their
 * offsets, kinds[4] (may be NULL) is incremented per block type (stored,
 * fixed, dynamic, literal-only dynamic).  0, -1 a payload too long, -2 dst
 * too small, -3 the emitted bits differ from the priced ones. */
int df_host_blocks(const uint8_t *buf, const int64_t *offs, int64_t n_blk, uint8_t *dst, int64_t dst_cap,
                   int64_t *dst_offs, int64_t kinds[4]);
/* the code-length builder alone (bgzfdef.h, df_build_lengths): n <= 288 */
void df_host_lengths(const uint32_t *freq, int n, int limit, int force_two, uint8_t *len);


/* Internal (vcfsort.hip): the stream written so far flushed as if at close,
 * then coff[0, n_blk) = every block's offset in the file and coff[n_blk] =
 * the offset the EOF marker will have.  Only close may follow.  The number of
 * blocks, or a negative GROM_E_* code (cap < n_blk + 1: GROM_E_ARG). */
struct grom_bgzf_writer;
int64_t grom_bgzf_writer_block_offsets(struct grom_bgzf_writer *w, int64_t *coff, int64_t cap);

#ifdef __cplusplus
}
#endif
