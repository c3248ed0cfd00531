// deflate_check.cpp -- the BGZF compressor's host twin (bgzfdef_host.cpp:
// bgzfdef.h's phases with the lanes as loops) against zlib's decoder, built
// under sanitizers (make sanitize; SAN=asan) and run as a plain executable.
// The grid of lengths and contents at which the compressor takes another
// path, every payload in a heap buffer that ends where the payload ends and
// every output buffer exactly as large as the blocks (a load or store past
// either is a sanitizer report); then the code-length builder alone on a
// Fibonacci histogram and on 1-, 2- and 286-symbol histograms.  No HIP, no
// device.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <string>
#include <vector>

#include "../grom_amd/csrc/bgzfwrite.h"
#include "../include/grom_amd.h"

static char g_last[4600];
extern "C" void grom_set_last_error(const char *m) { snprintf(g_last, sizeof(g_last), "%s", m ? m : ""); }

static int fails = 0;
#define CHECK(c, ...)                     \
    do {                                  \
        if (!(c)) {                       \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            fails++;                      \
        }                                 \
    } while (0)

static uint32_t g_x = 2463534242u;
static uint32_t rnd() {
    g_x = g_x * 1664525u + 1013904223u;
    return g_x >> 8;
}

// one payload, alone in its heap buffer, through the twin; its block checked.  Returns BTYPE or -1
static int one(const char *name, const std::vector<uint8_t> &payload) {
    const int64_t n = (int64_t)payload.size();
    uint8_t *in = (uint8_t *)malloc((size_t)n ? (size_t)n : 1);  // (the buffer ends where the payload ends)
    if (n) memcpy(in, payload.data(), (size_t)n);
    int64_t offs[2] = {0, n}, doffs[2] = {0, 0}, kinds[4] = {0, 0, 0, 0};
    // first into a large buffer for the size, then into one of exactly that size
    std::vector<uint8_t> big((size_t)n + 64);
    int rc = df_host_blocks(in, offs, 1, big.data(), (int64_t)big.size(), doffs, kinds);
    CHECK(rc == 0, "%s: twin returned %d", name, rc);
    if (rc != 0) { free(in); return -1; }
    const int64_t size = doffs[1];
    CHECK(size <= n + 31 && size >= 28, "%s: %lld bytes for a payload of %lld", name, (long long)size, (long long)n);
    uint8_t *out = (uint8_t *)malloc((size_t)size);
    rc = df_host_blocks(in, offs, 1, out, size, doffs, nullptr);
    CHECK(rc == 0 && doffs[1] == size && memcmp(out, big.data(), (size_t)size) == 0, "%s: the exact-size run differs (%d)", name, rc);
    CHECK(df_host_blocks(in, offs, 1, out, size - 1, doffs, nullptr) == -2, "%s: a short dst is not refused", name);
    static const uint8_t hdr[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    CHECK(memcmp(out, hdr, 16) == 0, "%s: header", name);
    CHECK((int64_t)(out[16] | out[17] << 8) == size - 1, "%s: BSIZE", name);
    const uint8_t *t = out + size - 8;
    const uint32_t crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
    const uint32_t isz = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
    CHECK(isz == (uint32_t)n, "%s: ISIZE %u", name, isz);
    CHECK(crc == (uint32_t)crc32(crc32(0L, Z_NULL, 0), in, (uInt)n), "%s: CRC-32", name);
    std::vector<uint8_t> back((size_t)n + 16);
    z_stream z;
    memset(&z, 0, sizeof(z));
    if (inflateInit2(&z, -15) != Z_OK) abort();
    z.next_in = out + 18;
    z.avail_in = (uInt)(size - 26);
    z.next_out = back.data();
    z.avail_out = (uInt)back.size();
    const int zr = inflate(&z, Z_FINISH);
    CHECK(zr == Z_STREAM_END && (int64_t)z.total_out == n && z.avail_in == 0 && (n == 0 || memcmp(back.data(), in, (size_t)n) == 0),
          "%s: zlib's inflate: %d, %lu of %lld bytes, %u input bytes left", name, zr, z.total_out, (long long)n, z.avail_in);
    inflateEnd(&z);
    const int btype = (out[18] >> 1) & 3;
    CHECK((out[18] & 1) == 1, "%s: not one final block", name);
    CHECK(kinds[0] + kinds[1] + kinds[2] + kinds[3] == 1 && (btype == 0) == (kinds[0] == 1) && (btype == 1) == (kinds[1] == 1),
          "%s: the kinds", name);
    free(out);
    free(in);
    return btype;
}

static std::vector<uint8_t> filled(size_t n, int fill) {
    std::vector<uint8_t> v(n);
    for (uint8_t &b : v) b = fill == 0 ? (uint8_t)rnd() : fill == 1 ? 0x00 : 0xff;
    return v;
}

static void lengths_case(const char *name, const std::vector<uint32_t> &freq, int limit, int force_two) {
    const int n = (int)freq.size();
    std::vector<uint8_t> len((size_t)n);  // (exactly n: a store past it is a report)
    df_host_lengths(freq.data(), n, limit, force_two, len.data());
    int used = 0, coded = 0;
    uint64_t kraft = 0;
    for (int i = 0; i < n; i++) {
        used += freq[(size_t)i] != 0;
        coded += len[(size_t)i] != 0;
        CHECK(len[(size_t)i] <= limit, "%s: symbol %d has %d bits (limit %d)", name, i, len[(size_t)i], limit);
        CHECK(freq[(size_t)i] == 0 || len[(size_t)i] != 0, "%s: used symbol %d has no code", name, i);
        if (len[(size_t)i]) kraft += (uint64_t)1 << (limit - len[(size_t)i]);
    }
    if (coded >= 2) CHECK(kraft == (uint64_t)1 << limit, "%s: Kraft sum %llu / %llu", name, (unsigned long long)kraft, 1ull << limit);
    if (used >= 2) CHECK(coded == used, "%s: %d codes for %d used symbols", name, coded, used);
    if (used == 1 && !force_two) CHECK(coded == 1 && kraft == (uint64_t)1 << (limit - 1), "%s: one symbol must take one bit", name);
    if (used <= 1 && force_two) CHECK(coded == 2, "%s: %d codes with a second one forced", name, coded);
    if (used == 0 && !force_two) CHECK(coded == 0, "%s: codes for an empty histogram", name);
}

int main() {
    long cases = 0;
    static const size_t lens[] = {0, 1, 2, 3, 4, 257, 258, 259, 260, 32767, 32768, 32769, 65279, 65280};
    char name[96];
    for (size_t n : lens)
        for (int fill = 0; fill < 3; fill++) {
            snprintf(name, sizeof(name), "n=%zu fill=%d", n, fill);
            const int bt = one(name, filled(n, fill));
            if (n == 65280 && fill == 0) CHECK(bt == 0, "%s: a random payload is not stored (BTYPE %d)", name, bt);
            cases++;
        }
    one("letter x1", std::vector<uint8_t>(1, 'A'));
    one("letter x2", std::vector<uint8_t>(2, 'A'));
    cases += 2;
    static const size_t periods[] = {1, 2, 3, 4, 32767, 32768, 32769};
    for (size_t p : periods) {
        const std::vector<uint8_t> base = filled(p, 0);
        std::vector<uint8_t> v(65280);
        for (size_t i = 0; i < v.size(); i++) v[i] = base[i % p];
        snprintf(name, sizeof(name), "period %zu", p);
        one(name, v);
        cases++;
    }
    {  // a copy of every length 3..258, then copies at every distance code's first distance and at 32768
        const std::vector<uint8_t> s = filled(259, 0);
        std::vector<uint8_t> v(s);
        for (size_t n = 3; n <= 258; n++) {
            v.insert(v.end(), s.begin(), s.begin() + (long)n);
            v.push_back((uint8_t)(s[n] ^ 0xff));
        }
        static const size_t firsts[] = {1,   2,   3,    4,    5,    7,    9,    13,   17,   25,    33,    49,    65,   97,  129, 193,
                                        257, 385, 513,  769,  1025, 1537, 2049, 3073, 4097, 6145,  8193,  12289, 16385, 24577, 32768};
        for (size_t d : firsts) {
            const size_t src = v.size() - d;
            for (size_t k = 0; k < 8; k++) v.push_back(v[src + k % d]);
            for (int k = 0; k < 3; k++) v.push_back((uint8_t)rnd());
        }
        CHECK(v.size() <= 65280 && v.size() > 32768, "copies: %zu bytes", v.size());
        one("copies", v);
        cases++;
    }
    std::vector<uint32_t> fib(22);
    {  // byte k occurs F(k + 1) times, shuffled: an unlimited Huffman tree is deeper than 15
        fib[0] = fib[1] = 1;
        for (size_t k = 2; k < 22; k++) fib[k] = fib[k - 1] + fib[k - 2];
        std::vector<uint8_t> v;
        for (size_t k = 0; k < 22; k++) v.insert(v.end(), fib[k], (uint8_t)(65 + k));
        CHECK(v.size() == 46367, "fibonacci: %zu bytes", v.size());
        for (size_t i = v.size() - 1; i > 0; i--) std::swap(v[i], v[rnd() % (i + 1)]);
        CHECK(one("fibonacci", v) == 2, "fibonacci: not a dynamic block");
        cases++;
    }
    {  // text: a four-letter sequence in lines, and tab-separated rows
        std::vector<uint8_t> v;
        for (int i = 0; v.size() < 65280; i++) v.push_back((i % 61) == 60 ? '\n' : (uint8_t) "ACGT"[rnd() & 3]);
        CHECK(one("acgt", v) == 2, "acgt: not a dynamic block");
        std::string t;
        for (int i = 0; t.size() < 60000; i++) {
            char row[160];
            snprintf(row, sizeof(row), "chr%d\t%u\t.\t%c\t%c\t.\tPASS\tDP=%u;AF=0.%u\tGT:PR\t0/1:%u\n", 1 + i % 3, 1000 + 37 * (unsigned)i,
                     "ACGT"[rnd() & 3], "ACGT"[rnd() & 3], rnd() % 90, rnd() % 1000, rnd() % 50);
            t += row;
        }
        CHECK(one("rows", std::vector<uint8_t>(t.begin(), t.end())) == 2, "rows: not a dynamic block");
        cases += 2;
    }
    // several payloads in one call, at every start alignment
    {
        const std::vector<uint8_t> v = filled(4000, 0);
        std::vector<int64_t> offs;
        for (int64_t o = 0; o + 200 <= (int64_t)v.size(); o += 200 + (int64_t)offs.size() % 16) offs.push_back(o);
        const int64_t nb = (int64_t)offs.size() - 1;
        std::vector<int64_t> doffs((size_t)nb + 1);
        std::vector<uint8_t> dst((size_t)(offs[(size_t)nb] - offs[0] + 31 * nb));
        const int rc = df_host_blocks(v.data(), offs.data(), nb, dst.data(), (int64_t)dst.size(), doffs.data(), nullptr);
        CHECK(rc == 0 && doffs[(size_t)nb] <= (int64_t)dst.size(), "many payloads: %d", rc);
        cases++;
    }
    // the code-length builder alone
    {
        std::vector<uint32_t> f(286, 0);
        for (size_t k = 0; k < 22; k++) f[65 + k] = fib[k];
        f[256] = 1;
        lengths_case("fibonacci/15", f, 15, 1);
        std::vector<uint32_t> f19(19, 0);
        for (size_t k = 0; k < 19; k++) f19[k] = fib[k];
        lengths_case("fibonacci/7", f19, 7, 1);
        std::vector<uint32_t> one_sym(286, 0);
        one_sym[256] = 1;
        lengths_case("one symbol, forced", one_sym, 15, 1);
        std::vector<uint32_t> d1(30, 0);
        lengths_case("no distance", d1, 15, 0);
        d1[29] = 7;
        lengths_case("one distance", d1, 15, 0);
        std::vector<uint32_t> two(286, 0);
        two[65] = 65280;
        two[256] = 1;
        lengths_case("two symbols", two, 15, 1);
        std::vector<uint32_t> all(286);
        for (size_t k = 0; k < 286; k++) all[k] = 1 + rnd() % 400;
        lengths_case("286 symbols", all, 15, 1);
        for (size_t k = 0; k < 286; k++) all[k] = 1;
        lengths_case("286 equal symbols", all, 15, 1);
        for (size_t k = 0; k < 286; k++) all[k] = k < 40 ? fib[k % 22] * 3 + 1 : 1;
        lengths_case("286 skewed symbols", all, 15, 1);
        std::vector<uint32_t> cl(19);
        for (size_t k = 0; k < 19; k++) cl[k] = 1u << k;
        lengths_case("19 powers of two / 7", cl, 7, 1);
        cases += 10;
    }
    if (fails) {
        fprintf(stderr, "deflate_check: %d failures\n", fails);
        return 1;
    }
    printf("deflate_check: ok (%ld cases)\n", cases);
    return 0;
}
