// gzipdev.h -- one plain gzip stream inflated on the device (gzipdev.hip,
// DESIGN.md 4.7.1); called by fastadev.hip for a file that is gzip but not BGZF.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// the defaults of GROM_GZIP_CHUNK_KB and GROM_GZIP_UNIT_MAX_KB
#define GZ_DEFAULT_CHUNK_KB 16.0
#define GZ_DEFAULT_UNIT_MAX_KB 256.0
// ms[]: guess, count/verify, symbolic decode, hand-over, resolve, CRC (HIP events)
#define GZ_DEV_STAGES 6

// comp: the file's n bytes in device memory, followed by 64 zero bytes.  On
// success 0 and *text (an allocation of *text_cap = size + text_pad bytes,
// accounted as decode memory, the caller's to free), *size, stats (the host
// twin's, grom_gzip_inflate_host) and the stage times.  GROM_FASTA_HOST_ONLY
// for a unit over the cap, else a negative GROM_E_* code with a message in err.
int gz_dev_read(hipStream_t st, const uint8_t *comp, int64_t n, size_t text_pad, uint8_t **text, size_t *text_cap,
                int64_t *size, int64_t stats[8], double ms[GZ_DEV_STAGES], char *err, size_t errn);
