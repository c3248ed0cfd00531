// crc_check.cpp -- the BGZF checksum kernel's host twin (bgzfcrc_host.cpp:
// bgzfcrc.h's table build, per-lane partials and combine with the lanes as a
// loop) against zlib's crc32, built under sanitizers (make sanitize; SAN=asan)
// and run as a plain executable.  Every length of the grid at every start
// alignment 0..15 with random, all-0x00 and all-0xff bytes, each block in a
// heap buffer that ends where the block ends (a load past it is a sanitizer
// report), then a BGZF file written here through grom_bgzf_check, whole and
// with one stored CRC bit flipped.  No HIP, no device.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#include <string>
#include <vector>

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

static void put_block(std::vector<uint8_t> &f, const uint8_t *p, uint32_t n, int level) {
    std::vector<uint8_t> c(n + 1024);
    z_stream z;
    memset(&z, 0, sizeof(z));
    if (deflateInit2(&z, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) abort();
    z.next_in = (Bytef *)p;
    z.avail_in = n;
    z.next_out = c.data();
    z.avail_out = (uInt)c.size();
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) abort();
    const uint32_t clen = (uint32_t)z.total_out, bsize = clen + 25, crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), p, n);
    deflateEnd(&z);
    const uint8_t h[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8)};
    f.insert(f.end(), h, h + 18);
    f.insert(f.end(), c.begin(), c.begin() + clen);
    for (int k = 0; k < 4; k++) f.push_back((uint8_t)(crc >> (8 * k)));
    for (int k = 0; k < 4; k++) f.push_back((uint8_t)(n >> (8 * k)));
}

int main() {
    static const uint32_t lens[] = {0,    1,    15,   16,   17,   63,   64,    65,    1007,  1008, 1023,
                                    1024, 1025, 2047, 2048, 2049, 4093, 65279, 65280, 65535, 65536};
    uint32_t x = 12345;
    long cases = 0;
    for (uint32_t n : lens)
        for (int a = 0; a < 16; a++)
            for (int fill = 0; fill < 3; fill++) {
                // the block is the buffer's last n bytes: the buffer ends where the block ends
                std::vector<uint8_t> buf((size_t)a + n);
                for (size_t i = 0; i < buf.size(); i++) {
                    x = x * 1664525u + 1013904223u;
                    buf[i] = fill == 0 ? (uint8_t)(x >> 24) : fill == 1 ? 0x00 : 0xff;
                }
                for (int i = 0; i < a; i++) buf[(size_t)i] = (uint8_t)(0xa5 ^ i);  // (bytes before the block must not count)
                const uint32_t want = (uint32_t)crc32(crc32(0L, Z_NULL, 0), buf.data() + a, n);
                const uint32_t got = grom_bgzf_crc_twin(buf.data(), (int64_t)buf.size(), a, n);
                CHECK(got == want, "crc twin: n=%u align=%d fill=%d: %08x, zlib %08x", n, a, fill, got, want);
                cases++;
            }
    // a block in the middle of a buffer (bytes after it must not count either)
    {
        std::vector<uint8_t> buf(70000);
        for (uint8_t &b : buf) {
            x = x * 1664525u + 1013904223u;
            b = (uint8_t)(x >> 24);
        }
        for (uint32_t n : lens) {
            if (n > 60000) continue;
            for (int a = 0; a < 16; a++) {
                const uint32_t want = (uint32_t)crc32(crc32(0L, Z_NULL, 0), buf.data() + 4000 + a, n);
                const uint32_t got = grom_bgzf_crc_twin(buf.data(), (int64_t)buf.size(), 4000 + a, n);
                CHECK(got == want, "crc twin (inner): n=%u align=%d: %08x, zlib %08x", n, a, got, want);
                cases++;
            }
        }
    }
    // the file check: a small BGZF file, whole and damaged
    {
        std::vector<uint8_t> f, data(65280);
        for (uint8_t &b : data) {
            x = x * 1664525u + 1013904223u;
            b = (uint8_t)"ACGT"[x >> 30];
        }
        std::vector<int64_t> offs;
        const uint32_t sizes[] = {65280, 1, 0, 4093, 17};
        const int levels[] = {1, 0, 1, 0, 6};
        for (int k = 0; k < 5; k++) {
            offs.push_back((int64_t)f.size());
            put_block(f, data.data(), sizes[k], levels[k]);
        }
        put_block(f, data.data(), 0, 6);  // (zlib's empty block: the 28-byte EOF marker)
        char path[] = "/tmp/crc_check_XXXXXX";
        const int fd = mkstemp(path);
        if (fd < 0) abort();
        auto write_all = [&](const std::vector<uint8_t> &v) {
            FILE *fp = fopen(path, "wb");
            if (!fp || fwrite(v.data(), 1, v.size(), fp) != v.size()) abort();
            fclose(fp);
        };
        int64_t out[8], bad[4];
        write_all(f);
        int rc = grom_bgzf_check(path, out, bad, 4);
        CHECK(rc == 0 && out[0] == 6 && out[1] == 0 && out[2] == -1 && out[3] == 65280 + 1 + 4093 + 17 && out[5] == 1,
              "file check (good): rc %d, %lld blocks, %lld bad, eof %lld: %s", rc, (long long)out[0], (long long)out[1],
              (long long)out[5], g_last);
        std::vector<uint8_t> g = f;
        g[(size_t)offs[2] - 8] ^= 0x10;  // block 1's stored CRC
        g[(size_t)offs[4] - 5] ^= 0x01;  // block 3's
        g.resize(g.size() - 28);         // and no EOF marker
        write_all(g);
        rc = grom_bgzf_check(path, out, bad, 4);
        CHECK(rc == GROM_E_ARG && out[0] == 5 && out[1] == 2 && out[2] == offs[1] && bad[0] == offs[1] && bad[1] == offs[3] &&
                  out[5] == 0 && strstr(g_last, "CRC-32 mismatch") != nullptr,
              "file check (damaged): rc %d, %lld blocks, %lld bad, first %lld: %s", rc, (long long)out[0], (long long)out[1],
              (long long)out[2], g_last);
        g.resize(g.size() - 3);  // a file that ends inside a block
        write_all(g);
        rc = grom_bgzf_check(path, out, bad, 4);
        CHECK(rc == GROM_E_ARG && strstr(g_last, "no whole BGZF block") != nullptr, "file check (cut): rc %d: %s", rc, g_last);
        close(fd);
        unlink(path);
    }
    if (fails) {
        fprintf(stderr, "crc_check: %d failures\n", fails);
        return 1;
    }
    printf("crc_check: ok (%ld buffers)\n", cases);
    return 0;
}
