// gzip_check.cpp -- the parallel gzip read's host twin (gzip_host.cpp) on
// good and damaged streams, built under sanitizers (make sanitize; SAN=asan)
// and run as a plain executable: every good stream gives zlib's bytes at
// every chunk size and guess mode, every damaged one an error code, and the
// sanitizers stay silent.  No HIP, no device.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <string>
#include <vector>

#include "../include/grom_amd.h"

extern "C" void grom_set_last_error(const char *) {}

typedef std::vector<uint8_t> Bytes;

// DNA-like lines with repeats, so that matches reach far back
static Bytes make_text(size_t n, uint32_t seed) {
    Bytes t;
    uint32_t x = seed;
    while (t.size() < n) {
        if (t.size() % 61 == 60) { t.push_back('\n'); continue; }
        x = x * 1664525u + 1013904223u;
        if ((x >> 24) < 8 && t.size() > 5000) {  // a copy of an earlier stretch
            const size_t from = (x >> 4) % (t.size() - 400), len = 100 + (x & 255);
            for (size_t i = 0; i < len && t.size() < n; i++) t.push_back(t[from + i]);
        } else {
            t.push_back("ACGTNacgtn"[(x >> 16) % ((x >> 28) ? 4 : 10)]);
        }
    }
    return t;
}

static Bytes gz(const Bytes &t, int level, int mem, int strategy, const char *name = nullptr) {
    z_stream z;
    memset(&z, 0, sizeof(z));
    if (deflateInit2(&z, level, Z_DEFLATED, 31, mem, strategy) != Z_OK) abort();
    gz_header h;
    memset(&h, 0, sizeof(h));
    if (name) {
        h.name = (Bytef *)name;
        h.comment = (Bytef *)"a comment";
        h.extra = (Bytef *)"xtra";
        h.extra_len = 4;
        h.hcrc = 1;
        deflateSetHeader(&z, &h);
    }
    Bytes out(deflateBound(&z, (uLong)t.size()) + 256);
    z.next_in = (Bytef *)t.data();
    z.avail_in = (uInt)t.size();
    z.next_out = out.data();
    z.avail_out = (uInt)out.size();
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) abort();
    out.resize(z.total_out);
    deflateEnd(&z);
    return out;
}

static int fails = 0;

// the twin's answer: 0 with the expected bytes, or an error code
static int run(const Bytes &s, const Bytes *want, int64_t chunk, int64_t cap, int mode) {
    uint8_t *out = nullptr;
    int64_t n = 0, st[8];
    const int rc = grom_gzip_inflate_host(s.data(), (int64_t)s.size(), chunk, cap, mode, &out, &n, st);
    int ok = rc;
    if (rc == 0 && want && (n != (int64_t)want->size() || memcmp(out, want->data(), (size_t)n) != 0)) ok = 1000;
    grom_gzip_free(out);
    return ok;
}

static void good(const char *what, const Bytes &s, const Bytes &want) {
    const int64_t chunks[] = {0, 4096, 1024, 256, 97};
    for (int64_t c : chunks)
        for (int mode = 0; mode < 3; mode++) {
            const int rc = run(s, &want, c, 0, mode);
            if (rc != 0) {
                printf("gzip_check: %s at chunk %lld mode %d: %d\n", what, (long long)c, mode, rc);
                fails++;
            }
        }
}

static void bad(const char *what, const Bytes &s, int64_t chunk = 256) {
    for (int mode = 0; mode < 3; mode++) {
        const int rc = run(s, nullptr, chunk, 0, mode);
        if (rc == 0) {
            printf("gzip_check: %s (mode %d) was accepted\n", what, mode);
            fails++;
        }
    }
}

int main() {
    const Bytes text = make_text(90000, 7);
    const Bytes m1 = gz(text, 6, 1, Z_DEFAULT_STRATEGY);  // many small blocks
    good("level 6", gz(text, 6, 8, Z_DEFAULT_STRATEGY), text);
    good("level 1", gz(text, 1, 8, Z_DEFAULT_STRATEGY), text);
    good("stored", gz(text, 0, 8, Z_DEFAULT_STRATEGY), text);
    good("fixed", gz(text, 6, 8, Z_FIXED), text);
    good("memLevel 1", m1, text);
    {  // three members, the middle one empty, header fields set
        const size_t cut = text.size() / 3;
        const Bytes a(text.begin(), text.begin() + (long)cut), c(text.begin() + (long)cut, text.end());
        Bytes s = gz(a, 6, 1, Z_DEFAULT_STRATEGY, "first.fa");
        const Bytes e = gz(Bytes(), 6, 8, Z_DEFAULT_STRATEGY), l = gz(c, 6, 1, Z_DEFAULT_STRATEGY, "last.fa");
        s.insert(s.end(), e.begin(), e.end());
        s.insert(s.end(), l.begin(), l.end());
        good("three members", s, text);
        Bytes g = s;  // trailing garbage after the last member
        for (int i = 0; i < 37; i++) g.push_back((uint8_t)(i * 37 + 1));
        bad("trailing garbage", g);
    }
    // cut at every 997th byte
    for (size_t cut = 1; cut < m1.size(); cut += 997) bad("a cut stream", Bytes(m1.begin(), m1.begin() + (long)cut));
    // the last block missing: the stream up to the trailer's place, then the trailer
    {
        Bytes s(m1.begin(), m1.end() - 8 - 200);
        s.insert(s.end(), m1.end() - 8, m1.end());
        bad("the last block missing", s);
    }
    // a bit flipped in a block header (the first block's HLIT) and in the member header
    {
        Bytes s = m1;
        s[10] ^= 0x10;
        bad("a flipped bit in a block header", s);
        s = m1;
        s[2] ^= 1;
        bad("a flipped bit in the member header", s);
        s = m1;
        s[m1.size() / 2] ^= 0x04;  // somewhere in the data: the CRC, the length or the decode catches it
        bad("a flipped bit in the data", s);
    }
    // a distance that points before the member's start: a fixed block whose first symbol is a match
    {
        // BFINAL 1, BTYPE 01, length code 257 (len 3: 0000001), distance code 0 (dist 1: 00000), end of block (0000000)
        const uint8_t body[] = {0x03 | 0x00, 0x02, 0x00, 0x00};  // bits: 1 10 0000001 00000 0000000
        Bytes s = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};
        s.insert(s.end(), body, body + 4);
        for (int i = 0; i < 8; i++) s.push_back(i == 4 ? 3 : 0);
        bad("a distance before the member's start", s);
        // the same in a second member, whose window must not reach into the first
        Bytes two = gz(text, 6, 8, Z_DEFAULT_STRATEGY);
        two.insert(two.end(), s.begin(), s.end());
        bad("a distance into the member before", two);
    }
    // wrong trailer fields on a valid stream
    {
        Bytes s = m1;
        s[s.size() - 8] ^= 0xff;
        bad("a wrong CRC-32", s);
        s = m1;
        s[s.size() - 4] ^= 0x01;
        bad("a wrong ISIZE", s);
    }
    // the unit cap: a fixed-block stream has no start to guess
    if (run(gz(text, 6, 8, Z_FIXED), nullptr, 1024, 4096, 1) != GROM_FASTA_HOST_ONLY) {
        printf("gzip_check: the unit cap did not answer host only\n");
        fails++;
    }
    if (fails) {
        printf("gzip_check: %d failures\n", fails);
        return 1;
    }
    printf("gzip_check ok\n");
    return 0;
}
