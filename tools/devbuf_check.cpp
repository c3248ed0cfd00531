// devbuf_check.cpp -- the growable device buffer (grom_amd/csrc/devbuf.h) on
// the host: grom_dev_malloc, grom_dev_free and grom_arena_take are defined
// here on top of malloc and record every call, so the sizes a DevBuf asks
// for, what it frees and when can be checked without HIP or a device.
// Built with AddressSanitizer + UBSan by `make sanitize` (tests/test_devbuf.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "../grom_amd/csrc/devbuf.h"

namespace {

struct Call {
    int cat;
    size_t bytes;
};
std::vector<Call> g_mallocs, g_frees;
std::map<void *, Call> g_live;  // blocks allocated and not yet freed
int64_t g_live_bytes = 0;
int g_fail = 0;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            fprintf(stderr, "devbuf_check:%d: %s\n", __LINE__, #c);    \
            g_fail++;                                                  \
        }                                                              \
    } while (0)

}  // namespace

struct grom_arena {
    char block[8192];
    size_t room, used = 0;
    explicit grom_arena(size_t r) : room(r) {}
};

extern "C" int grom_dev_malloc(void **p, size_t bytes, int cat) {
    g_mallocs.push_back({cat, bytes});
    *p = malloc(1);  // (sizes up to 64 MB are asked for: only the size is recorded)
    g_live[*p] = {cat, bytes};
    g_live_bytes += (int64_t)bytes;
    return 0;
}

extern "C" void grom_dev_free(void *p, size_t bytes, int cat) {
    g_frees.push_back({cat, bytes});
    auto it = g_live.find(p);
    CHECK(it != g_live.end());  // freed exactly once, and a block of ours
    if (it == g_live.end()) return;
    CHECK(it->second.bytes == bytes && it->second.cat == cat);
    g_live_bytes -= (int64_t)it->second.bytes;
    g_live.erase(it);
    free(p);
}

extern "C" void *grom_arena_take(grom_arena *a, size_t bytes) {
    if (a->used + bytes > a->room) return nullptr;
    void *p = a->block + a->used;
    a->used += bytes;
    return p;
}

namespace {

// the sizes each module's buffers asked of the allocator before devbuf.h
// (scan.hip, sv.hip: bytes/8 + 64; cnv.hip, baidev.hip, fastadev.hip:
// bytes/8 + 256; ddecode.hip: bytes/64 + 256 from 64 MB on), written out
template <class B> void check_sizes(int cat, bool with_64mb, const size_t (&req)[5], const size_t (&want)[5]) {
    for (int k = 0; k < (with_64mb ? 5 : 4); k++) {
        const size_t n0 = g_mallocs.size();
        {
            B b;
            CHECK(b.grow(req[k]) == 0);
            CHECK(g_mallocs.size() == n0 + 1);
            CHECK(g_mallocs.back().bytes == want[k] && g_mallocs.back().cat == cat);
            CHECK(b.cap == want[k] && b.own && b.p != nullptr);
            CHECK(b.want(req[k]) == want[k]);
        }
        CHECK(g_frees.back().bytes == want[k] && g_frees.back().cat == cat);
    }
}

const size_t REQ[5] = {0, 1, 4096, ((size_t)64 << 20) - 1, (size_t)64 << 20};

void sizes() {
    // request 0 becomes 16; (64 << 20) - 1 = 67108863, / 8 = 8388607; 64 << 20 = 67108864, / 64 = 1048576
    const size_t pad64[5] = {16 + 2 + 64, 1 + 0 + 64, 4096 + 512 + 64, 67108863 + 8388607 + 64, 0};
    const size_t pad256[5] = {16 + 2 + 256, 1 + 0 + 256, 4096 + 512 + 256, 67108863 + 8388607 + 256, 0};
    const size_t taper[5] = {16 + 2 + 256, 1 + 0 + 256, 4096 + 512 + 256, 67108863 + 8388607 + 256,
                             67108864 + 1048576 + 256};
    check_sizes<DevBufOf<GROM_DEVCAT_SCAN, 64>>(GROM_DEVCAT_SCAN, false, REQ, pad64);             // scan.hip
    check_sizes<DevBufOf<GROM_DEVCAT_SV, 64>>(GROM_DEVCAT_SV, false, REQ, pad64);                 // sv.hip
    check_sizes<DevBufOf<GROM_DEVCAT_CNV, 256>>(GROM_DEVCAT_CNV, false, REQ, pad256);             // cnv.hip
    check_sizes<DevBufOf<GROM_DEVCAT_DECODE, 256, true>>(GROM_DEVCAT_DECODE, true, REQ, taper);   // ddecode.hip
    check_sizes<DevBufOf<GROM_DEVCAT_DECODE, 256>>(GROM_DEVCAT_DECODE, false, REQ, pad256);       // baidev, fastadev
}

using Buf = DevBufOf<GROM_DEVCAT_SV, 64>;

void regrow() {
    Buf b;
    CHECK(b.grow(1000) == 0);
    const size_t cap0 = b.cap, nm = g_mallocs.size(), nf = g_frees.size();
    CHECK(cap0 == 1000 + 125 + 64);
    CHECK(b.grow(10) == 0 && b.grow(0) == 0 && b.grow(cap0) == 0);  // smaller, or what it holds: nothing allocated
    CHECK(g_mallocs.size() == nm && g_frees.size() == nf && b.cap == cap0);
    CHECK(b.grow(cap0 + 1) == 0);  // a regrow frees the old block with its old capacity and category
    CHECK(g_frees.size() == nf + 1 && g_frees.back().bytes == cap0 && g_frees.back().cat == GROM_DEVCAT_SV);
    CHECK(g_mallocs.size() == nm + 1 && b.cap == (cap0 + 1) + (cap0 + 1) / 8 + 64);
}

void arena() {
    const size_t nm = g_mallocs.size(), nf = g_frees.size();
    grom_arena room(4096), full(0);
    {
        Buf b;
        b.rebind(&room);
        CHECK(b.grow(100) == 0);
        CHECK(!b.own && b.p == room.block && b.cap == 100 + 12 + 64 && g_mallocs.size() == nm);
    }
    CHECK(g_frees.size() == nf);  // a piece of the arena: nothing to free
    {
        Buf b;
        b.rebind(&full);
        CHECK(b.grow(100) == 0);  // the arena is full: an allocation of its own
        CHECK(b.own && b.cap == 100 + 12 + 64 && g_mallocs.size() == nm + 1);
    }
    CHECK(g_frees.size() == nf + 1 && g_frees.back().bytes == 100 + 12 + 64);
}

void rebind() {
    grom_arena room(4096), full(0);
    Buf b;
    // an own overflow block, a new phase with an arena: freed
    b.rebind(&full);
    CHECK(b.grow(100) == 0 && b.own);
    size_t nf = g_frees.size();
    b.rebind(&room);
    CHECK(g_frees.size() == nf + 1 && b.p == nullptr && b.cap == 0 && !b.own && b.ar == &room);
    // a piece of the arena, a new phase (with or without an arena): dropped, nothing freed
    CHECK(b.grow(100) == 0 && !b.own);
    b.rebind(&room);
    CHECK(g_frees.size() == nf + 1 && b.p == nullptr && b.cap == 0 && !b.own);
    CHECK(b.grow(100) == 0 && !b.own);
    b.rebind(nullptr);
    CHECK(g_frees.size() == nf + 1 && b.p == nullptr && b.cap == 0 && b.ar == nullptr);
    // an own block, a new phase without an arena: it stays
    CHECK(b.grow(100) == 0 && b.own);
    void *p = b.p;
    b.rebind(nullptr);
    CHECK(g_frees.size() == nf + 1 && b.p == p && b.cap == 100 + 12 + 64 && b.own);
}

void moves() {
    Buf a;
    CHECK(a.grow(100) == 0);
    void *p = a.p;
    const size_t cap = a.cap, nf = g_frees.size();
    Buf b(std::move(a));
    CHECK(a.p == nullptr && a.cap == 0 && !a.own);
    CHECK(b.p == p && b.cap == cap && b.own && g_frees.size() == nf);
    Buf c;
    CHECK(c.grow(7) == 0);
    c = std::move(b);  // the target's old block is freed, the source left empty
    CHECK(g_frees.size() == nf + 1 && g_frees.back().bytes == 7 + 0 + 64);
    CHECK(b.p == nullptr && b.cap == 0 && !b.own && c.p == p && c.cap == cap && c.own);
    CHECK(P<char>(c) == (char *)p);
}

}  // namespace

int main() {
    sizes();
    regrow();
    arena();
    rebind();
    moves();
    // every buffer is gone: nothing live, every block freed exactly once
    CHECK(g_live.empty() && g_live_bytes == 0);
    CHECK(g_mallocs.size() == g_frees.size());
    if (g_fail) {
        fprintf(stderr, "devbuf_check: %d checks failed\n", g_fail);
        return 1;
    }
    printf("devbuf_check: ok (%zu allocations)\n", g_mallocs.size());
    return 0;
}
