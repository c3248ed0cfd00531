// fastadev.hip -- the reference FASTA read on the device.
//
// The file's bytes are brought to the device once: a BGZF (bgzip) file is read
// in whole blocks through two pinned buffers into HBM (DdBgzfFile, ddecode.h,
// which also builds each read's block table) and its blocks inflated by the
// decoder's inflater (dd_inflate_launch, one block per lane) into one resident
// text; a plain file is copied as it is; a plain gzip file (one DEFLATE stream
// per member; GROM_FASTA_GZIP=1) is copied as it is and inflated by gzipdev.hip.  The index (grom_fasta_open,
// stream.c) and the loader (grom_fasta_load) are then kernels over that text,
// and give the host code's results bit for bit.  The scratch of those kernels
// is DevBufs (devbuf.h) accounted as decode memory, freed with the handle; the
// text and the loaded references are plain allocations of their exact size.
//
// The host code reads with fgets(line, 1000).  Written without the sequential
// read: a segment starts where reading starts or after a '\n'; a chunk starts
// at every position q with (q - segment_start(q)) % 999 == 0 and runs to the
// next chunk start.  The text is scanned in pieces (GROM_FASTA_PIECE_KB); a
// piece ends at its last chunk start, which begins the next piece as a new
// segment (q - q = 0: the chunking after it is the same), so no line is too
// long for a piece.  Per piece:
//   k_fa_tile    per 4 KB tile: the last newline, a NUL byte seen
//   (max-scan over tiles: the segment start every tile begins in)
//   k_fa_starts  per tile: the chunk starts counted, then written compactly
//   k_fa_chunk   per chunk: header?, letters, letters other than N, the
//                loader's cut (measure) keyed by the chunk index where the
//                length changes
//   (max-scan of the keys: the cut in effect; sums of the counts)
//   k_fa_alpha   per chunk: the bytes it contributes
//   k_fa_hdr     the header chunks gathered for the host's name rule
//   k_fa_copy    the reference written contiguously, 16 bytes per lane
// The bytes are arbitrary user text: every load is bounded by the piece.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "../../include/grom_amd.h"
#include "bamio.h"
#include "ddecode.h"
#include "devbuf.h"
#include "gzipdev.h"
#include "stream.h"

namespace {

#define FA_TPB 256
#define FA_BPT 16                  // bytes per lane: one 16-byte load
#define FA_TILE (FA_TPB * FA_BPT)  // 4096
#define FA_LINE 999                // fgets(line, 1000)
#define FA_HDR_SLOT 1000           // a gathered header chunk's bytes
#define FA_TEXT_PAD 8192           // readable bytes past the text (whole tiles are loaded)

__device__ __forceinline__ bool fa_alpha(uint8_t c) { return (uint32_t)((c | 32u) - 'a') < 26u; }

// the window: text bytes T[a0 + i], i in [lo, n); a0 is 16-byte aligned and
// lo < 16 is where the window (a segment) starts

// per tile: the segment start its last newline opens (INT_MIN: none); flag bit 0: a NUL byte
__global__ void __launch_bounds__(FA_TPB) k_fa_tile(const uint8_t *__restrict__ T, int64_t a0, int lo, int n,
                                                    int *__restrict__ tile_seg, uint32_t *__restrict__ flags) {
    typedef hipcub::BlockReduce<int, FA_TPB> Red;
    __shared__ typename Red::TempStorage tmp;
    const int i0 = (int)blockIdx.x * FA_TILE + (int)threadIdx.x * FA_BPT;
    int v = INT_MIN;
    bool nul = false;
    if (i0 < n) {
        const uint4 w = *(const uint4 *)(T + a0 + i0);
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < FA_BPT; k++) {
            const int i = i0 + k;
            const uint8_t c = (uint8_t)(ws[k >> 2] >> (8 * (k & 3)));
            if (i >= lo && i < n) {
                if (c == '\n') v = i + 1;
                nul = nul || c == 0;
            }
        }
    }
    if (nul) atomicOr(flags, 1u);
    const int m = Red(tmp).Reduce(v, hipcub::Max());
    if (threadIdx.x == 0) tile_seg[blockIdx.x] = m;
}

// per tile: its chunk starts counted (WRITE false: tile_cnt) or written
// (WRITE true: cs[tile_base[tile] + ...]); tile_segs is the inclusive max-scan
// of tile_seg
template <bool WRITE>
__global__ void __launch_bounds__(FA_TPB) k_fa_starts(const uint8_t *__restrict__ T, int64_t a0, int lo, int n,
                                                      const int *__restrict__ tile_segs,
                                                      uint32_t *__restrict__ tile_cnt,
                                                      const uint32_t *__restrict__ tile_base, int *__restrict__ cs,
                                                      int64_t cs_cap) {
    typedef hipcub::BlockScan<int, FA_TPB> Scan;
    __shared__ typename Scan::TempStorage tmp_a, tmp_b;
    const int b = (int)blockIdx.x;
    const int i0 = b * FA_TILE + (int)threadIdx.x * FA_BPT;
    uint32_t ws[4] = {0, 0, 0, 0};
    if (i0 < n) {
        const uint4 w = *(const uint4 *)(T + a0 + i0);
        ws[0] = w.x; ws[1] = w.y; ws[2] = w.z; ws[3] = w.w;
    }
    int v = INT_MIN;
#pragma unroll
    for (int k = 0; k < FA_BPT; k++) {
        const int i = i0 + k;
        if (i >= lo && i < n && (uint8_t)(ws[k >> 2] >> (8 * (k & 3))) == '\n') v = i + 1;
    }
    int pre;
    Scan(tmp_a).ExclusiveScan(v, pre, INT_MIN, hipcub::Max());
    int cin = lo;
    if (b > 0) cin = max(cin, tile_segs[b - 1]);
    const int seg = max(cin, pre);
    // the starts among this lane's bytes
    uint32_t mask = 0;
    int d = -1;
#pragma unroll
    for (int k = 0; k < FA_BPT; k++) {
        const int i = i0 + k;
        if (i < lo || i >= n) continue;
        if (d < 0) d = (i - seg) % FA_LINE;
        if (d == 0) mask |= 1u << k;
        d++;
        if (d == FA_LINE || (uint8_t)(ws[k >> 2] >> (8 * (k & 3))) == '\n') d = 0;
    }
    const int cnt = __popc(mask);
    int at, total;
    Scan(tmp_b).ExclusiveSum(cnt, at, total);
    if (!WRITE) {
        if (threadIdx.x == 0) tile_cnt[b] = (uint32_t)total;
        return;
    }
    int64_t o = (int64_t)tile_base[b] + at;
    for (uint32_t m = mask; m; m &= m - 1, o++)
        if (o < cs_cap) cs[o] = i0 + __builtin_ctz(m);
}

struct FaCarry {
    int prev_l;  // the last chunk's length
    int alpha;   // the cut in effect after it
    int first;   // the next chunk is an entry's first (the last chunk was a header)
    int pad;
};

// per chunk k < nproc (cs[nproc] is the end of the last one): header flag,
// letter counts (counts != 0) and the key of the "last flagged value" scan:
// (k + 1) << 32 | measure where the cut is measured again -- an entry's first
// chunk, or a length that differs from the chunk before
__global__ void k_fa_chunk(const uint8_t *__restrict__ T, int64_t a0, const int *__restrict__ cs, int64_t nproc,
                           int counts, FaCarry cin, uint8_t *__restrict__ hdr, uint64_t *__restrict__ ca,
                           uint64_t *__restrict__ cn, uint64_t *__restrict__ key) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nproc) return;
    if (k == nproc) {  // the scans' last element
        hdr[k] = 0;
        ca[k] = cn[k] = key[k] = 0;
        return;
    }
    const int p = cs[k], L = cs[k + 1] - p;
    const uint8_t *s = T + a0 + p;
    const bool h = s[0] == '>';
    uint32_t na = 0, nn = 0;
    if (counts && !h)
        for (int i = 0; i < L; i++) {
            const uint8_t c = s[i];
            const bool al = fa_alpha(c);
            na += al;
            nn += al && c != 'N' && c != 'n';
        }
    uint64_t ky = 0;
    if (!h) {
        bool flag;
        if (k == 0) flag = cin.first || L != cin.prev_l;
        else {
            const int q = cs[k - 1];
            flag = T[a0 + q] == '>' || L != p - q;
        }
        if (flag) {
            int w = L - 1;
            while (w > 0 && !fa_alpha(s[w])) w--;
            ky = ((uint64_t)(k + 1) << 32) | (uint32_t)(w + 1);
        }
    }
    hdr[k] = h;
    ca[k] = na;
    cn[k] = nn;
    key[k] = ky;
}

// ks = the inclusive max-scan of key: the bytes chunk k contributes
__global__ void k_fa_alpha(const int *__restrict__ cs, int64_t nproc, const uint8_t *__restrict__ hdr,
                           const uint64_t *__restrict__ ks, FaCarry cin, uint64_t *__restrict__ al,
                           FaCarry *__restrict__ cout) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nproc) return;
    if (k == nproc) { al[k] = 0; return; }
    const uint64_t s = ks[k];
    const int a = s ? (int)(uint32_t)s : cin.alpha;
    al[k] = hdr[k] ? 0 : (uint64_t)a;
    if (k == nproc - 1) {
        FaCarry c;
        c.prev_l = cs[k + 1] - cs[k];
        c.alpha = a;
        c.first = hdr[k];
        c.pad = 0;
        *cout = c;
    }
}

struct FaHdr {
    int64_t pos;  // the chunk's first byte in the window
    int64_t L;
    uint64_t pa, pl;  // letters / loader bytes before it in the window
};

// header j (chunk hidx[j]): its facts and its first FA_HDR_SLOT - 1 bytes
__global__ void __launch_bounds__(64) k_fa_hdr(const uint8_t *__restrict__ T, int64_t a0, const int *__restrict__ cs,
                                               const int *__restrict__ hidx, int nh, int64_t nproc,
                                               const uint64_t *__restrict__ pa, const uint64_t *__restrict__ pl,
                                               FaHdr *__restrict__ rec, uint8_t *__restrict__ hbuf) {
    const int j = (int)blockIdx.x;
    if (j >= nh) return;
    const int64_t k = hidx[j];
    if (k < 0 || k >= nproc) return;
    const int p = cs[k], L = cs[k + 1] - p;
    if (threadIdx.x == 0) {
        FaHdr r;
        r.pos = p;
        r.L = L;
        r.pa = pa[k];
        r.pl = pl[k];
        rec[j] = r;
    }
    const int m = L < FA_HDR_SLOT - 1 ? L : FA_HDR_SLOT - 1;
    for (int i = (int)threadIdx.x; i < FA_HDR_SLOT; i += 64) hbuf[(size_t)j * FA_HDR_SLOT + i] = i < m ? T[a0 + p + i] : 0;
}

// the loaded bytes: out[obase + pl[k] ...] = the first al[k] bytes of chunk
// k < nlim (pl strictly increasing: every chunk gives at least one byte).
// One lane per 16 aligned output bytes: a binary search finds the chunk of the
// first byte, the lane walks on from there and stores once
__global__ void k_fa_copy(const uint8_t *__restrict__ T, int64_t a0, const int *__restrict__ cs,
                          const uint64_t *__restrict__ pl, int64_t nlim, uint8_t *__restrict__ out, int64_t obase,
                          int64_t wl) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t A = obase & ~(int64_t)15;
    int64_t o0 = A + 16 * g, o1 = o0 + 16;
    if (o0 >= obase + wl) return;
    const bool full = o0 >= obase && o1 <= obase + wl;
    if (o0 < obase) o0 = obase;
    if (o1 > obase + wl) o1 = obase + wl;
    uint64_t r = (uint64_t)(o0 - obase);
    int64_t lo = 0, hi = nlim;  // the last k with pl[k] <= r
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (pl[mid] <= r) lo = mid;
        else hi = mid;
    }
    int64_t k = lo;
    uint64_t base = pl[k], next = pl[k + 1];
    const uint8_t *s = T + a0 + cs[k];
    uint8_t b[16];
    const int cnt = (int)(o1 - o0);
    for (int i = 0; i < 16; i++) {
        if (i >= cnt) break;
        while (r >= next && k + 1 < nlim) {
            k++;
            base = next;
            next = pl[k + 1];
            s = T + a0 + cs[k];
        }
        b[i] = s[r - base];
        r++;
    }
    if (full) {
        uint4 w;
        w.x = b[0] | b[1] << 8 | b[2] << 16 | (uint32_t)b[3] << 24;
        w.y = b[4] | b[5] << 8 | b[6] << 16 | (uint32_t)b[7] << 24;
        w.z = b[8] | b[9] << 8 | b[10] << 16 | (uint32_t)b[11] << 24;
        w.w = b[12] | b[13] << 8 | b[14] << 16 | (uint32_t)b[15] << 24;
        *(uint4 *)(out + o0) = w;
    } else {
        for (int i = 0; i < cnt; i++) out[o0 + i] = b[i];
    }
}

using Buf = DevBufOf<GROM_DEVCAT_DECODE, 256>;  // decode memory, an eighth of slack (devbuf.h)

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct Entry {
    char name[GROM_MAX_CHR_NAME_LEN];
    int name_len;
    int64_t file_pos, len, load_len;
};

// what one piece gave
struct Win {
    int64_t a0 = 0, nproc = 0, next = 0;
    bool last = false;
    int nh = 0;
    uint64_t tot_a = 0, tot_n = 0, tot_l = 0;
};

}  // namespace

// the kernels' scratch (a base of its own: grom_fasta_dev_close releases it in one assignment)
struct FaScratch {
    Buf tile_seg, tile_segs, tile_cnt, tile_base, cs, hdr, ca, cn, key, ks, al, pa, pn, pl, hidx, nsel, hrec, hbuf, small,
        tmp;
};

struct grom_fasta_dev : FaScratch {
    int device = 0, bgzf = 0;
    int kind = 0;  // grom_fasta_file_kind: 0 plain text, 1 BGZF, 2 gzip that is not BGZF
    int64_t gz_stats[8] = {};
    double gz_ms[GZ_DEV_STAGES] = {};
    int64_t piece = (int64_t)256 << 20;
    int64_t size = 0;  // the text's bytes
    uint8_t *text = nullptr;
    size_t text_cap = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev[2] = {};
    int64_t *h_small = nullptr;  // pinned
    std::vector<Entry> ent;
    int64_t mappable = 0;
    bool indexed = false;
    std::vector<FaHdr> h_rec;
    std::vector<uint8_t> h_hdr;
    std::vector<std::pair<void *, size_t>> refs;  // loaded references not yet released
    double ms[8] = {};
    char err[512] = {0};

    int fail(int code, const char *fmt, long long a = 0, long long b = 0) {
        snprintf(err, sizeof(err), fmt, a, b);
        return code;
    }
};

#define FAK(x)                                                                                                     \
    do {                                                                                                           \
        hipError_t e_ = (x);                                                                                       \
        if (e_ != hipSuccess) {                                                                                    \
            snprintf(d->err, sizeof(d->err), "device FASTA: HIP error %s at %s:%d", hipGetErrorString(e_), __FILE__, \
                     __LINE__);                                                                                    \
            return GROM_E_HIP;                                                                                     \
        }                                                                                                          \
    } while (0)
#define FAG(b, bytes)                                                                                              \
    do {                                                                                                           \
        if ((b).grow(bytes)) return d->fail(GROM_E_NOMEM, "device FASTA: hipMalloc(%lld) failed", (long long)(bytes)); \
    } while (0)

namespace {

void tic(grom_fasta_dev *d) { (void)hipEventRecord(d->ev[0], d->st); }
// waits for the stream; the HIP-event time since tic added to *acc
int toc(grom_fasta_dev *d, double *acc) {
    FAK(hipEventRecord(d->ev[1], d->st));
    FAK(hipEventSynchronize(d->ev[1]));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, d->ev[0], d->ev[1]);
    *acc += ms;
    return 0;
}

// the file's bytes to the device: the text itself, or BGZF blocks inflated
int ingest(grom_fasta_dev *d, const char *path) {
    const double t0 = now_ms();
    DdBgzfFile R(path);  // (the plain file too: its FILE and ring buffers)
    if (!R.fp) return d->fail(GROM_E_ARG, "device FASTA: the file does not open");
    FILE *fp = R.fp;
    const int64_t fsize = R.size;
    // a ring buffer is read into again once its last copy is done
    struct Events {
        hipEvent_t rev[2] = {};
        ~Events() {
            for (hipEvent_t e : rev)
                if (e) (void)hipEventDestroy(e);
        }
    } E;
    const int64_t ring = std::min<int64_t>(std::max<int64_t>(d->piece, 131072), (int64_t)64 << 20);
    FAK((hipError_t)R.rings(ring, d->bgzf ? (size_t)(ring / 64 + 64) : 0));  // (a plain file has no block table)
    for (int k = 0; k < 2; k++) FAK(hipEventCreateWithFlags(&E.rev[k], hipEventDisableTiming));
    Buf comp;
    if (!d->bgzf) {
        // the file as it is: the text itself, or (gzip) the stream to inflate
        uint8_t *dst = nullptr;
        if (d->kind == 2) {
            FAG(comp, (size_t)fsize + 64);
            dst = P<uint8_t>(comp);
            FAK(hipMemsetAsync(dst + fsize, 0, 64, d->st));
        } else {
            d->size = fsize;
            d->text_cap = (size_t)fsize + FA_TEXT_PAD;
            if (grom_dev_malloc((void **)&d->text, d->text_cap, GROM_DEVCAT_DECODE) != 0)
                return d->fail(GROM_E_NOMEM, "device FASTA: hipMalloc(%lld) failed", (long long)d->text_cap);
            dst = d->text;
        }
        int64_t off = 0;
        for (int64_t k = 0; off < fsize; k++) {
            const int s = (int)(k & 1);
            if (k >= 2) FAK(hipEventSynchronize(E.rev[s]));
            const int64_t want = std::min<int64_t>(ring, fsize - off);
            if ((int64_t)fread(R.ring[s], 1, (size_t)want, fp) != want)
                return d->fail(GROM_E_ARG, "device FASTA: read error at byte %lld", (long long)off);
            FAK(hipMemcpyAsync(dst + off, R.ring[s], (size_t)want, hipMemcpyHostToDevice, d->st));
            FAK(hipEventRecord(E.rev[s], d->st));
            off += want;
        }
        FAK(hipStreamSynchronize(d->st));
        d->ms[0] += now_ms() - t0;
        if (d->kind != 2) return 0;
        // one DEFLATE stream per member, read in parallel (gzipdev.hip); its
        // scratch is freed when gz_dev_read returns, the compressed copy with `comp`
        const int rc = gz_dev_read(d->st, dst, fsize, FA_TEXT_PAD, &d->text, &d->text_cap, &d->size, d->gz_stats, d->gz_ms,
                                   d->err, sizeof(d->err));
        d->gz_stats[6] += (int64_t)comp.cap;
        for (int k = 0; k < GZ_DEV_STAGES; k++) d->ms[1] += d->gz_ms[k];
        return rc;
    }
    // BGZF: the compressed file to HBM in whole blocks, the block table beside it
    Buf dblk, status, tok, misc;
    FAG(comp, (size_t)fsize + 64);
    std::vector<DdBlock> all;
    int64_t total = 0;
    for (int64_t k = 0; R.off < fsize; k++) {
        const int s = (int)(k & 1);
        if (k >= 2) FAK(hipEventSynchronize(E.rev[s]));
        const int64_t foff = R.off;
        int64_t clen = 0, ub = 0;  // (ub: not needed, the blocks are summed below)
        const int64_t n = R.read(s, INT64_MAX, &clen, &ub);
        if (n == DD_READ_IO) return d->fail(GROM_E_ARG, "device FASTA: read error at byte %lld", (long long)foff);
        if (n <= 0) return d->fail(GROM_E_ARG, "device FASTA: no whole BGZF block at byte %lld", (long long)foff);
        for (int64_t i = 0; i < n; i++) {
            DdBlock b = R.tab[(size_t)i];
            b.in_off += foff;
            b.c_off += foff;
            b.out_off = total;
            total += b.out_len;
            all.push_back(b);
        }
        FAK(hipMemcpyAsync(P<uint8_t>(comp) + foff, R.ring[s], (size_t)clen, hipMemcpyHostToDevice, d->st));
        FAK(hipEventRecord(E.rev[s], d->st));
    }
    FAK(hipMemsetAsync(P<uint8_t>(comp) + fsize, 0, 64, d->st));
    FAK(hipStreamSynchronize(d->st));
    d->ms[0] += now_ms() - t0;
    d->size = total;
    d->text_cap = (size_t)total + FA_TEXT_PAD;
    if (grom_dev_malloc((void **)&d->text, d->text_cap, GROM_DEVCAT_DECODE) != 0)
        return d->fail(GROM_E_NOMEM, "device FASTA: hipMalloc(%lld) failed", (long long)d->text_cap);
    const int64_t nb = (int64_t)all.size();
    FAG(dblk, sizeof(DdBlock) * (size_t)(nb + 1));
    FAG(status, (size_t)nb + 16);
    FAG(misc, 64);
    FAK(hipMemcpyAsync(dblk.p, all.data(), sizeof(DdBlock) * (size_t)nb, hipMemcpyHostToDevice, d->st));
    FAK(hipMemsetAsync(misc.p, 0, 64, d->st));
    uint32_t *m32 = P<uint32_t>(misc);  // [0] blocks that did not inflate, [1] bounds, [2] CRCs that differ, [3] the first
    const bool verify = bgzf_verify_on() != 0;  // (read once per open)
    if (verify) FAK(hipMemsetAsync(m32 + 3, 0xff, 4, d->st));
    tic(d);
    // One block per lane: a launch's time hardly depends on the number of
    // blocks, and the text is resident, so every block goes in one launch
    // (with GROM_FASTA_PIECE_KB set: as many as a piece holds)
    const int64_t per_launch = getenv("GROM_FASTA_PIECE_KB") ? d->piece : INT64_MAX;
    for (int64_t b0 = 0; b0 < nb;) {
        int64_t b1 = b0, ub = 0;
        while (b1 < nb && (b1 == b0 || ub + all[(size_t)b1].out_len <= per_launch)) ub += all[(size_t)b1++].out_len;
        const size_t tokb = dd_inflate_tok_bytes(b1 - b0);
        if (tokb) FAG(tok, tokb);
        if (dd_inflate_launch(d->st, P<uint8_t>(comp), fsize, P<DdBlock>(dblk) + b0, b1 - b0, d->text, 0, total,
                              P<uint8_t>(status) + b0, m32, m32 + 1, tokb ? P<uint32_t>(tok) : nullptr, tokb ? tok.cap : 0))
            return d->fail(GROM_E_HIP, "device FASTA: the inflate launch failed");
        if (verify && dd_crc_launch(d->st, P<uint8_t>(comp), fsize, P<DdBlock>(dblk) + b0, b1 - b0, d->text, 0, total,
                                    P<uint8_t>(status) + b0, m32 + 2, m32 + 1, m32 + 3))
            return d->fail(GROM_E_HIP, "device FASTA: the CRC launch failed");
        b0 = b1;
    }
    FAK(hipMemcpyAsync(d->h_small, misc.p, 64, hipMemcpyDeviceToHost, d->st));
    if (toc(d, &d->ms[1])) return GROM_E_HIP;
    const uint32_t *h32 = (const uint32_t *)d->h_small;
    if (verify && h32[2]) {  // a hard error: the host reader would meet the same bytes
        int64_t foff = -1;
        if (per_launch == INT64_MAX) {
            foff = h32[3] < (uint64_t)nb ? all[(size_t)h32[3]].c_off : -1;
        } else {  // (launches of their own block ranges: the first block whose trailer differs, found on the host)
            std::vector<uint8_t> hs((size_t)nb);
            FAK(hipMemcpy(hs.data(), status.p, (size_t)nb, hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < nb && foff < 0; i++)
                if (hs[(size_t)i] == GI_E_CRC) foff = all[(size_t)i].c_off;
        }
        bgzf_crc_fail(path, foff);
        dd_crc_message(d->err, (int)sizeof(d->err), path, foff);
        return GROM_E_ARG;
    }
    if (h32[0] || h32[1]) return d->fail(GROM_E_ARG, "device FASTA: %lld BGZF blocks did not inflate", h32[0]);
    return 0;
}

// One piece of the text from `start` (a segment start), at most to `limit`:
// the chunk table and the per-chunk sums are left in the device buffers.
// counts: the index's letter counts too
int scan_piece(grom_fasta_dev *d, int64_t start, int64_t limit, int counts, FaCarry &carry, Win &w, double *acc,
               uint32_t *nul) {
    const int64_t a0 = start & ~(int64_t)15;
    const int lo = (int)(start - a0);
    const int64_t end = std::min<int64_t>(limit, start + d->piece);
    const int n = (int)(end - a0);
    w = Win();
    w.a0 = a0;
    w.last = end >= limit;
    const int ntile = (n + FA_TILE - 1) / FA_TILE;
    FAG(d->tile_seg, 4 * (size_t)ntile);
    FAG(d->tile_segs, 4 * (size_t)ntile);
    FAG(d->tile_cnt, 4 * (size_t)(ntile + 1));
    FAG(d->tile_base, 4 * (size_t)(ntile + 1));
    FAG(d->small, 256);
    size_t t1 = 0, t2 = 0;
    FAK(hipcub::DeviceScan::InclusiveScan(nullptr, t1, (int *)nullptr, (int *)nullptr, hipcub::Max(), ntile, d->st));
    FAK(hipcub::DeviceScan::ExclusiveSum(nullptr, t2, (uint32_t *)nullptr, (uint32_t *)nullptr, ntile + 1, d->st));
    FAG(d->tmp, std::max(t1, t2));
    uint32_t *flags = P<uint32_t>(d->small);
    FaCarry *d_carry = (FaCarry *)(P<uint8_t>(d->small) + 64);
    tic(d);
    FAK(hipMemsetAsync(d->small.p, 0, 256, d->st));
    hipLaunchKernelGGL(k_fa_tile, dim3((unsigned)ntile), dim3(FA_TPB), 0, d->st, d->text, a0, lo, n, P<int>(d->tile_seg), flags);
    size_t tb = d->tmp.cap;
    FAK(hipcub::DeviceScan::InclusiveScan(d->tmp.p, tb, P<int>(d->tile_seg), P<int>(d->tile_segs), hipcub::Max(), ntile, d->st));
    hipLaunchKernelGGL(k_fa_starts<false>, dim3((unsigned)ntile), dim3(FA_TPB), 0, d->st, d->text, a0, lo, n,
                       P<int>(d->tile_segs), P<uint32_t>(d->tile_cnt), (const uint32_t *)nullptr, (int *)nullptr, (int64_t)0);
    FAK(hipMemsetAsync(P<uint32_t>(d->tile_cnt) + ntile, 0, 4, d->st));
    tb = d->tmp.cap;
    FAK(hipcub::DeviceScan::ExclusiveSum(d->tmp.p, tb, P<uint32_t>(d->tile_cnt), P<uint32_t>(d->tile_base), ntile + 1, d->st));
    FAK(hipGetLastError());
    FAK(hipMemcpyAsync(d->h_small, P<uint32_t>(d->tile_base) + ntile, 4, hipMemcpyDeviceToHost, d->st));
    FAK(hipMemcpyAsync(d->h_small + 1, flags, 4, hipMemcpyDeviceToHost, d->st));
    if (toc(d, acc)) return GROM_E_HIP;
    const int64_t nc = (int64_t)(uint32_t)d->h_small[0];
    *nul = (uint32_t)d->h_small[1] & 1u;
    if (*nul) return 0;
    if (nc < 1 || (!w.last && nc < 2)) return d->fail(GROM_E_HIP, "device FASTA: a piece of %lld bytes has %lld chunks", n - lo, nc);
    const int64_t nproc = w.last ? nc : nc - 1;
    w.nproc = nproc;
    FAG(d->cs, 4 * (size_t)(nc + 1));
    const size_t n1 = (size_t)nproc + 1;
    FAG(d->hdr, n1);
    FAG(d->ca, 8 * n1);
    FAG(d->cn, 8 * n1);
    FAG(d->key, 8 * n1);
    FAG(d->ks, 8 * n1);
    FAG(d->al, 8 * n1);
    FAG(d->pa, 8 * n1);
    FAG(d->pn, 8 * n1);
    FAG(d->pl, 8 * n1);
    FAG(d->hidx, 4 * n1);
    FAG(d->nsel, 16);
    size_t t3 = 0, t4 = 0, t5 = 0;
    FAK(hipcub::DeviceScan::InclusiveScan(nullptr, t3, (uint64_t *)nullptr, (uint64_t *)nullptr, hipcub::Max(), (int)n1, d->st));
    FAK(hipcub::DeviceScan::ExclusiveSum(nullptr, t4, (uint64_t *)nullptr, (uint64_t *)nullptr, (int)n1, d->st));
    hipcub::CountingInputIterator<int> cnt_it(0);
    FAK(hipcub::DeviceSelect::Flagged(nullptr, t5, cnt_it, (uint8_t *)nullptr, (int *)nullptr, (int *)nullptr, (int)nproc, d->st));
    FAG(d->tmp, std::max(t3, std::max(t4, t5)));
    const unsigned gc = (unsigned)((n1 + 255) / 256);
    tic(d);
    hipLaunchKernelGGL(k_fa_starts<true>, dim3((unsigned)ntile), dim3(FA_TPB), 0, d->st, d->text, a0, lo, n,
                       P<int>(d->tile_segs), (uint32_t *)nullptr, P<uint32_t>(d->tile_base), P<int>(d->cs), nc);
    FAK(hipMemcpyAsync(P<int>(d->cs) + nc, &n, 4, hipMemcpyHostToDevice, d->st));
    hipLaunchKernelGGL(k_fa_chunk, dim3(gc), dim3(256), 0, d->st, d->text, a0, P<int>(d->cs), nproc, counts, carry,
                       P<uint8_t>(d->hdr), P<uint64_t>(d->ca), P<uint64_t>(d->cn), P<uint64_t>(d->key));
    tb = d->tmp.cap;
    FAK(hipcub::DeviceScan::InclusiveScan(d->tmp.p, tb, P<uint64_t>(d->key), P<uint64_t>(d->ks), hipcub::Max(), (int)n1, d->st));
    hipLaunchKernelGGL(k_fa_alpha, dim3(gc), dim3(256), 0, d->st, P<int>(d->cs), nproc, P<uint8_t>(d->hdr),
                       P<uint64_t>(d->ks), carry, P<uint64_t>(d->al), d_carry);
    FAK(hipGetLastError());
    tb = d->tmp.cap;
    FAK(hipcub::DeviceScan::ExclusiveSum(d->tmp.p, tb, P<uint64_t>(d->al), P<uint64_t>(d->pl), (int)n1, d->st));
    if (counts) {
        tb = d->tmp.cap;
        FAK(hipcub::DeviceScan::ExclusiveSum(d->tmp.p, tb, P<uint64_t>(d->ca), P<uint64_t>(d->pa), (int)n1, d->st));
        tb = d->tmp.cap;
        FAK(hipcub::DeviceScan::ExclusiveSum(d->tmp.p, tb, P<uint64_t>(d->cn), P<uint64_t>(d->pn), (int)n1, d->st));
    } else {
        FAK(hipMemsetAsync(P<uint64_t>(d->pa) + nproc, 0, 8, d->st));
        FAK(hipMemsetAsync(P<uint64_t>(d->pn) + nproc, 0, 8, d->st));
    }
    tb = d->tmp.cap;
    FAK(hipcub::DeviceSelect::Flagged(d->tmp.p, tb, cnt_it, P<uint8_t>(d->hdr), P<int>(d->hidx), P<int>(d->nsel), (int)nproc, d->st));
    FAK(hipMemcpyAsync(d->h_small, d->nsel.p, 4, hipMemcpyDeviceToHost, d->st));
    FAK(hipMemcpyAsync(d->h_small + 1, P<uint64_t>(d->pa) + nproc, 8, hipMemcpyDeviceToHost, d->st));
    FAK(hipMemcpyAsync(d->h_small + 2, P<uint64_t>(d->pn) + nproc, 8, hipMemcpyDeviceToHost, d->st));
    FAK(hipMemcpyAsync(d->h_small + 3, P<uint64_t>(d->pl) + nproc, 8, hipMemcpyDeviceToHost, d->st));
    FAK(hipMemcpyAsync(d->h_small + 4, P<int>(d->cs) + (nc - 1), 4, hipMemcpyDeviceToHost, d->st));
    FAK(hipMemcpyAsync(d->h_small + 5, d_carry, sizeof(FaCarry), hipMemcpyDeviceToHost, d->st));
    if (toc(d, acc)) return GROM_E_HIP;
    w.nh = (int)(int32_t)d->h_small[0];
    w.tot_a = (uint64_t)d->h_small[1];
    w.tot_n = (uint64_t)d->h_small[2];
    w.tot_l = (uint64_t)d->h_small[3];
    w.next = w.last ? limit : a0 + (int64_t)(int32_t)d->h_small[4];
    memcpy(&carry, d->h_small + 5, sizeof(FaCarry));
    if (!w.last && w.next <= start) return d->fail(GROM_E_HIP, "device FASTA: a piece made no progress at byte %lld", start);
    return 0;
}

// the first nh header chunks of the piece gathered to the host (h_rec, h_hdr)
int gather_headers(grom_fasta_dev *d, const Win &w, int nh, double *acc) {
    FAG(d->hrec, sizeof(FaHdr) * (size_t)nh);
    FAG(d->hbuf, (size_t)FA_HDR_SLOT * (size_t)nh);
    d->h_rec.resize((size_t)nh);
    d->h_hdr.resize((size_t)FA_HDR_SLOT * (size_t)nh);
    tic(d);
    hipLaunchKernelGGL(k_fa_hdr, dim3((unsigned)nh), dim3(64), 0, d->st, d->text, w.a0, P<int>(d->cs), P<int>(d->hidx), nh,
                       w.nproc, P<uint64_t>(d->pa), P<uint64_t>(d->pl), P<FaHdr>(d->hrec), P<uint8_t>(d->hbuf));
    FAK(hipGetLastError());
    FAK(hipMemcpyAsync(d->h_rec.data(), d->hrec.p, sizeof(FaHdr) * (size_t)nh, hipMemcpyDeviceToHost, d->st));
    FAK(hipMemcpyAsync(d->h_hdr.data(), d->hbuf.p, (size_t)FA_HDR_SLOT * (size_t)nh, hipMemcpyDeviceToHost, d->st));
    return toc(d, acc);
}

int set_dev(grom_fasta_dev *d) {
    FAK(hipSetDevice(d->device));
    return 0;
}

}  // namespace

extern "C" int grom_fasta_dev_open(const char *path, int device, grom_fasta_dev **out) {
    if (out) *out = nullptr;
    if (!path || !out) {
        grom_set_last_error("grom_fasta_dev_open: bad argument");
        return GROM_E_ARG;
    }
    const double t0 = now_ms();
    const int kind = grom_fasta_file_kind(path);
    char m[4600];
    if (kind < 0) {
        snprintf(m, sizeof(m), "grom_fasta_dev_open: %s does not open", path);
        grom_set_last_error(m);
        return GROM_E_ARG;
    }
    if (kind == 2 && !grom_fasta_gzip_allowed()) {
        snprintf(m, sizeof(m), "%s is gzip-compressed but not BGZF: recompress it with bgzip, or set GROM_FASTA_GZIP=1 to "
                 "read it as it is", path);
        grom_set_last_error(m);
        return GROM_E_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) {
        snprintf(m, sizeof(m), "grom_fasta_dev_open: no device %d (%d visible)", device, ndev);
        grom_set_last_error(m);
        return GROM_E_NODEV;
    }
    grom_fasta_dev *d = new grom_fasta_dev();
    d->device = device;
    d->bgzf = kind == 1;
    d->kind = kind;
    const char *e = getenv("GROM_FASTA_PIECE_KB");
    if (e && atof(e) > 0) d->piece = (int64_t)(atof(e) * 1024.0);
    d->piece = std::min<int64_t>(std::max<int64_t>(d->piece, 4096), (int64_t)1 << 30);
    int rc = [&]() -> int {
        FAK(hipStreamCreateWithFlags(&d->st, hipStreamNonBlocking));
        for (int k = 0; k < 2; k++) FAK(hipEventCreate(&d->ev[k]));
        FAK(hipHostMalloc((void **)&d->h_small, 32 * sizeof(int64_t), 0));
        return ingest(d, path);
    }();
    d->ms[5] = now_ms() - t0;
    if (rc != 0) {
        // (host only: a gzip unit over the cap -- the caller reads the file on the host)
        if (rc != GROM_FASTA_HOST_ONLY) {
            snprintf(m, sizeof(m), "%s (%s)", d->err[0] ? d->err : "device FASTA: open failed", path);
            grom_set_last_error(m);
        }
        grom_fasta_dev_close(d);
        return rc;
    }
    *out = d;
    return 0;
}

extern "C" void grom_fasta_dev_close(grom_fasta_dev *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    if (d->st) (void)hipStreamSynchronize(d->st);
    static_cast<FaScratch &>(*d) = FaScratch();
    for (auto &r : d->refs) grom_dev_free(r.first, r.second, GROM_DEVCAT_DECODE);
    if (d->text) grom_dev_free(d->text, d->text_cap, GROM_DEVCAT_DECODE);
    for (int k = 0; k < 2; k++)
        if (d->ev[k]) (void)hipEventDestroy(d->ev[k]);
    if (d->h_small) (void)hipHostFree(d->h_small);
    if (d->st) (void)hipStreamDestroy(d->st);
    delete d;
}

extern "C" int grom_fasta_dev_is_bgzf(const grom_fasta_dev *d) { return d ? d->bgzf : 0; }

extern "C" int grom_fasta_dev_kind(const grom_fasta_dev *d) { return d ? d->kind : -1; }

extern "C" void grom_fasta_dev_gzip_stats(const grom_fasta_dev *d, int64_t stats[8], double ms[6]) {
    for (int k = 0; k < 8; k++) stats[k] = d ? d->gz_stats[k] : 0;
    for (int k = 0; k < GZ_DEV_STAGES; k++) ms[k] = d ? d->gz_ms[k] : 0.0;
}

extern "C" int grom_fasta_dev_index(grom_fasta_dev *d, int *n_out, int64_t *mappable) {
    if (!d) { grom_set_last_error("grom_fasta_dev_index: null handle"); return GROM_E_ARG; }
    const double t0 = now_ms();
    int rc = [&]() -> int {
        if (set_dev(d)) return GROM_E_HIP;
        d->ent.clear();
        d->mappable = 0;
        d->indexed = false;
        FaCarry carry = {-1, 0, 1, 0};
        bool have = false;  // an entry is open
        int64_t start = 0;
        while (start < d->size) {
            Win w;
            uint32_t nul = 0;
            const int r = scan_piece(d, start, d->size, 1, carry, w, &d->ms[2], &nul);
            if (r) return r;
            if (nul) return GROM_FASTA_HOST_ONLY;
            if ((int64_t)d->ent.size() + w.nh > GROM_MAX_CHR_NAMES) return GROM_FASTA_HOST_ONLY;
            if (w.nh > 0 && gather_headers(d, w, w.nh, &d->ms[2])) return GROM_E_HIP;
            uint64_t a_mark = 0, l_mark = 0;
            for (int j = 0; j < w.nh; j++) {
                const FaHdr &h = d->h_rec[(size_t)j];
                if (have) {
                    d->ent.back().len += (int64_t)(h.pa - a_mark);
                    d->ent.back().load_len += (int64_t)(h.pl - l_mark);
                }
                Entry en;
                memset(&en, 0, sizeof(en));
                const int L = (int)std::min<int64_t>(h.L, FA_HDR_SLOT - 1);
                en.name_len = grom_fasta_header_name((const char *)d->h_hdr.data() + (size_t)j * FA_HDR_SLOT, L, en.name);
                en.file_pos = w.a0 + h.pos + h.L;
                d->ent.push_back(en);
                have = true;
                a_mark = h.pa;
                l_mark = h.pl;
            }
            if (have) {
                d->ent.back().len += (int64_t)(w.tot_a - a_mark);
                d->ent.back().load_len += (int64_t)(w.tot_l - l_mark);
            }
            d->mappable += (int64_t)w.tot_n;
            start = w.next;
        }
        d->indexed = true;
        return 0;
    }();
    d->ms[6] += now_ms() - t0;
    if (rc < 0 && rc != GROM_FASTA_HOST_ONLY) grom_set_last_error(d->err[0] ? d->err : "device FASTA: the index pass failed");
    if (rc == 0) {
        if (n_out) *n_out = (int)d->ent.size();
        if (mappable) *mappable = d->mappable;
    }
    return rc;
}

extern "C" int grom_fasta_dev_entry(const grom_fasta_dev *d, int i, char name[GROM_FASTA_NAME_LEN], int *name_len,
                                    int64_t *file_pos, int64_t *len, int64_t *load_len) {
    if (!d || !d->indexed || i < 0 || i >= (int)d->ent.size()) {
        grom_set_last_error("grom_fasta_dev_entry: no such entry");
        return GROM_E_ARG;
    }
    const Entry &e = d->ent[(size_t)i];
    if (name) memcpy(name, e.name, GROM_FASTA_NAME_LEN);
    if (name_len) *name_len = e.name_len;
    if (file_pos) *file_pos = e.file_pos;
    if (len) *len = e.len;
    if (load_len) *load_len = e.load_len;
    return 0;
}

extern "C" int grom_fasta_dev_set_index(grom_fasta_dev *d, int n, int64_t mappable, const char *names, const int *name_len,
                                        const int64_t *file_pos, const int64_t *len) {
    if (!d || n < 0 || n > GROM_MAX_CHR_NAMES || (n > 0 && (!names || !name_len || !file_pos || !len))) {
        grom_set_last_error("grom_fasta_dev_set_index: bad argument");
        return GROM_E_ARG;
    }
    for (int i = 0; i < n; i++)
        if (file_pos[i] < 0 || file_pos[i] > d->size) {
            grom_set_last_error("grom_fasta_dev_set_index: an entry's file_pos lies outside the text");
            return GROM_E_ARG;
        }
    d->ent.assign((size_t)n, Entry());
    for (int i = 0; i < n; i++) {
        Entry &e = d->ent[(size_t)i];
        memcpy(e.name, names + (size_t)i * GROM_FASTA_NAME_LEN, GROM_FASTA_NAME_LEN);
        e.name_len = name_len[i];
        e.file_pos = file_pos[i];
        e.len = len[i];
        e.load_len = -1;
    }
    d->mappable = mappable;
    d->indexed = true;
    return 0;
}

extern "C" int64_t grom_fasta_dev_load(grom_fasta_dev *d, int i, char *host_buf, int64_t cap, const void **dev_ptr) {
    if (dev_ptr) *dev_ptr = nullptr;
    if (!d || !d->indexed || i < 0 || i >= (int)d->ent.size() || cap < 0) {
        grom_set_last_error("grom_fasta_dev_load: no such entry");
        return GROM_E_ARG;
    }
    const double t0 = now_ms();
    uint8_t *ref = nullptr;
    size_t ref_cap = 0;
    int64_t rc = [&]() -> int64_t {
        if (set_dev(d)) return GROM_E_HIP;
        Entry &e = d->ent[(size_t)i];
        // the span ends before the next entry's file_pos (its header lies before that) or at the end of the text
        int64_t limit = d->size;
        for (const Entry &o : d->ent)
            if (o.file_pos > e.file_pos && o.file_pos < limit) limit = o.file_pos;
        // pass 0 measures the length (unless the index pass did), pass 1 copies
        for (int pass = e.load_len >= 0 ? 1 : 0; pass < 2; pass++) {
            if (pass == 1) {
                if (cap == 0) return e.load_len;
                if (cap < e.load_len) return d->fail(GROM_E_ARG, "grom_fasta_dev_load: the buffer holds %lld of %lld bytes", cap, e.load_len);
                ref_cap = (size_t)e.load_len + 64;
                if (grom_dev_malloc((void **)&ref, ref_cap, GROM_DEVCAT_DECODE) != 0)
                    return d->fail(GROM_E_NOMEM, "device FASTA: hipMalloc(%lld) failed", (long long)ref_cap);
            }
            FaCarry carry = {-1, 0, 1, 0};
            int64_t start = e.file_pos, len = 0;
            while (start < limit) {
                Win w;
                uint32_t nul = 0;
                const int r = scan_piece(d, start, limit, 0, carry, w, &d->ms[3], &nul);
                if (r) return r;
                if (nul) return GROM_FASTA_HOST_ONLY;
                int64_t nlim = w.nproc;
                uint64_t wl = w.tot_l;
                if (w.nh > 0) {  // the first header chunk ends the entry
                    if (gather_headers(d, w, 1, &d->ms[3])) return GROM_E_HIP;
                    wl = d->h_rec[0].pl;
                    FAK(hipMemcpyAsync(d->h_small, d->hidx.p, 4, hipMemcpyDeviceToHost, d->st));
                    FAK(hipStreamSynchronize(d->st));
                    nlim = (int64_t)(int32_t)d->h_small[0];
                }
                if (pass == 1 && wl > 0) {
                    if (len + (int64_t)wl > e.load_len) return d->fail(GROM_E_HIP, "device FASTA: entry %lld grew past its length", i);
                    const int64_t groups = (((len + (int64_t)wl + 15) >> 4) - (len >> 4));
                    tic(d);
                    hipLaunchKernelGGL(k_fa_copy, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, d->st, d->text, w.a0,
                                       P<int>(d->cs), P<uint64_t>(d->pl), nlim, ref, len, (int64_t)wl);
                    FAK(hipGetLastError());
                    if (toc(d, &d->ms[3])) return GROM_E_HIP;
                }
                len += (int64_t)wl;
                if (w.nh > 0) break;
                start = w.next;
            }
            if (pass == 0) e.load_len = len;
            else if (len != e.load_len) return d->fail(GROM_E_HIP, "device FASTA: entry %lld gave %lld bytes", i, len);
        }
        if (host_buf && e.load_len > 0) {
            const double t1 = now_ms();
            FAK(hipMemcpyAsync(host_buf, ref, (size_t)e.load_len, hipMemcpyDeviceToHost, d->st));
            FAK(hipStreamSynchronize(d->st));
            d->ms[4] += now_ms() - t1;
        }
        return e.load_len;
    }();
    d->ms[7] += now_ms() - t0;
    if (ref) {
        if (rc >= 0 && dev_ptr) {
            d->refs.push_back({ref, ref_cap});
            *dev_ptr = ref;
        } else {
            grom_dev_free(ref, ref_cap, GROM_DEVCAT_DECODE);
        }
    }
    if (rc < 0 && rc != GROM_FASTA_HOST_ONLY) grom_set_last_error(d->err[0] ? d->err : "device FASTA: the load failed");
    return rc;
}

extern "C" void grom_fasta_dev_release(grom_fasta_dev *d, const void *dev_ptr) {
    if (!d || !dev_ptr) return;
    (void)hipSetDevice(d->device);
    for (size_t k = 0; k < d->refs.size(); k++)
        if (d->refs[k].first == dev_ptr) {
            grom_dev_free(d->refs[k].first, d->refs[k].second, GROM_DEVCAT_DECODE);
            d->refs.erase(d->refs.begin() + (ptrdiff_t)k);
            return;
        }
}

extern "C" void grom_fasta_dev_times(const grom_fasta_dev *d, double ms[8]) {
    for (int k = 0; k < 8; k++) ms[k] = d ? d->ms[k] : 0.0;
}
