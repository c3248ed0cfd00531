// devbuf.h -- the one growable device buffer of the library.
//
// A DevBuf is a block of device memory that grows to the largest size asked
// of it and frees itself.  Every module's scratch is made of them: the scan
// context (scan.hip), the breakpoint and CNV scratch (sv.hip, cnv.hip), the
// BAM decoder (ddecode.hip), the index builder (baidev.hip) and the FASTA
// reader (fastadev.hip).  A module names its kind once,
//
//     using Buf = DevBufOf<GROM_DEVCAT_SV, 64>;
//
// which fixes the accounting category (devmem.h) and the growth slack: a
// request of `bytes` allocates bytes + bytes/8 + PAD (TAPER: bytes/64 + PAD
// from 64 MB on, for run-sized buffers reserved from estimates that carry
// their own margin).  The slack lets kernels read whole 16-byte words past
// the last element and spares a regrow for a slightly larger chromosome.
//
// With a phase arena bound (rebind; devmem.h, grom_arena) a buffer is first
// carved from the arena and does not own its memory; when the arena is full
// it overflows into an allocation of its own, which the next rebind frees.
//
// grow() returns 0 or -1 and writes no message: the caller words its own.
// Depends only on devmem.h; no HIP.
#pragma once
#include <stddef.h>

#include "devmem.h"

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    bool own = false;          // p is this buffer's own allocation (else a piece of `ar`'s phase)
    grom_arena *ar = nullptr;  // the owner's phase arena (rebind), or none
    int cat;                   // GROM_DEVCAT_*: what an own allocation is accounted under
    unsigned pad;              // the slack's constant part
    bool taper;                // the slack is bytes/64 instead of bytes/8 from 64 MB on

    DevBuf(int cat_, unsigned pad_, bool taper_ = false) : cat(cat_), pad(pad_), taper(taper_) {}
    ~DevBuf() { release(); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap), own(o.own), ar(o.ar), cat(o.cat), pad(o.pad), taper(o.taper) {
        o.forget();
    }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap, own = o.own, ar = o.ar, cat = o.cat, pad = o.pad, taper = o.taper;
            o.forget();
        }
        return *this;
    }

    // the bytes a request of `bytes` allocates
    size_t want(size_t bytes) const {
        if (bytes == 0) bytes = 16;
        return bytes + (taper && bytes >= ((size_t)64 << 20) ? bytes / 64 : bytes / 8) + pad;
    }

    // room for `bytes` (0: 16); the contents are lost when it has to grow.  0 or -1
    int grow(size_t bytes) {
        if (bytes == 0) bytes = 16;
        if (cap >= bytes) return 0;
        release();
        const size_t w = want(bytes);
        if (ar && (p = grom_arena_take(ar, w)) != nullptr) {
            cap = w;
            return 0;
        }
        if (grom_dev_malloc(&p, w, cat) != 0) {
            p = nullptr;
            return -1;
        }
        cap = w;
        own = true;
        return 0;
    }

    // a new phase of the owner: the arena's last phase is dead, so a piece of
    // it is dropped and an overflow of the last phase freed; without an arena
    // the buffer's own allocation stays
    void rebind(grom_arena *a) {
        if (!own || a) release();
        ar = a;
    }

    // empty again; an own allocation is freed
    void release() {
        if (p && own) grom_dev_free(p, cap, cat);
        forget();
    }

private:
    void forget() {
        p = nullptr;
        cap = 0;
        own = false;
    }
};

// a module's kind of DevBuf: default-constructible, so it can be a plain member
template <int CAT, unsigned PAD, bool TAPER = false> struct DevBufOf : DevBuf {
    DevBufOf() : DevBuf(CAT, PAD, TAPER) {}
};

template <class T> T *P(DevBuf &b) { return (T *)b.p; }
