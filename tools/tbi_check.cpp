// tbi_check.cpp -- the sorting, indexing VCF writer's host twin
// (vcfsort_host.cpp: vcfsort.h's per-row arithmetic in loops, the .tbi
// through bamio.c's accumulator) built under sanitizers (make sanitize;
// SAN=asan) and run as a plain executable.
//
//   tbi_check DIR [MORE.vcf ...]
//
// Every DIR/*.vcf, each read into a heap buffer that ends where the text
// ends (a load past it is a sanitizer report), goes through vs_host_run to
// DIR/NAME.vcf.gz, .tbi and .gzi; zlib reads the files back: the data file
// must inflate to the input's header and as many bytes and lines as the
// input, with non-decreasing POS inside each contig, and the .tbi to "TBI\1".
// A DIR/refused_*.vcf must be refused with a message and leave no file.  The
// MORE files (the golden VCF) go the same way, written into DIR.  No HIP, no
// device.
#include <dirent.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../grom_amd/csrc/vcfsort_host.h"
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

static bool slurp_gz(const std::string &path, std::vector<uint8_t> &out) {
    gzFile g = gzopen(path.c_str(), "rb");
    if (!g) return false;
    out.clear();
    std::vector<uint8_t> buf(1 << 16);
    int k;
    while ((k = gzread(g, buf.data(), (unsigned)buf.size())) > 0) out.insert(out.end(), buf.begin(), buf.begin() + k);
    gzclose(g);
    return k == 0;
}

static bool exists(const std::string &p) { return access(p.c_str(), F_OK) == 0; }

static void one(const std::string &src, const std::string &dst, bool refused) {
    FILE *f = fopen(src.c_str(), "rb");
    CHECK(f, "%s: cannot open", src.c_str());
    if (!f) return;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t *text = (uint8_t *)malloc(n > 0 ? (size_t)n : 1);  // (the buffer ends where the text ends)
    CHECK(n == 0 || fread(text, 1, (size_t)n, f) == (size_t)n, "%s: short read", src.c_str());
    fclose(f);
    int64_t out[12];
    char err[512] = {0};
    const int rc = vs_host_run(text, n, dst.c_str(), out, err, sizeof(err));
    if (refused) {
        CHECK(rc != 0 && strncmp(err, "VCF sort: ", 10) == 0, "%s: not refused (%d, %s)", src.c_str(), rc, err);
        CHECK(!exists(dst) && !exists(dst + ".tbi") && !exists(dst + ".gzi"), "%s: a refusal left a file", src.c_str());
        free(text);
        return;
    }
    CHECK(rc == 0, "%s: %d %s", src.c_str(), rc, err);
    std::vector<uint8_t> back, tbi;
    CHECK(slurp_gz(dst, back), "%s: zlib cannot read the data file", dst.c_str());
    CHECK(slurp_gz(dst + ".tbi", tbi), "%s: zlib cannot read the .tbi", dst.c_str());
    CHECK(exists(dst + ".gzi"), "%s: no .gzi", dst.c_str());
    CHECK(tbi.size() >= 44 && memcmp(tbi.data(), "TBI\1", 4) == 0, "%s: the .tbi's magic", dst.c_str());
    CHECK((long)back.size() == n, "%s: %zu bytes back for %ld", dst.c_str(), back.size(), n);
    if ((long)back.size() == n && rc == 0) {
        // the header in place, the same number of lines, POS non-decreasing inside a contig, contigs not repeated
        long hb = 0, lines_in = 0, lines_out = 0;
        while (hb < n && text[hb] == '#') {
            while (text[hb] != '\n') hb++;
            hb++;
        }
        CHECK(memcmp(back.data(), text, (size_t)hb) == 0, "%s: the header moved", dst.c_str());
        for (long i = 0; i < n; i++) lines_in += text[i] == '\n', lines_out += back[(size_t)i] == '\n';
        CHECK(lines_in == lines_out, "%s: lines", dst.c_str());
        std::map<std::string, int> seen;
        std::string cur;
        long long last = -1, rows = 0;
        for (long a = hb; a < n;) {
            long t1 = a;
            while (back[(size_t)t1] != '\t') t1++;
            std::string nm((const char *)&back[(size_t)a], (size_t)(t1 - a));
            const long long pos = atoll((const char *)&back[(size_t)t1 + 1]);
            if (nm != cur) {
                CHECK(seen.count(nm) == 0, "%s: contig %s comes twice", dst.c_str(), nm.c_str());
                seen[nm] = 1;
                cur = nm;
                last = -1;
            }
            CHECK(pos >= last, "%s: POS %lld after %lld", dst.c_str(), pos, last);
            last = pos;
            rows++;
            while (back[(size_t)a] != '\n') a++;
            a++;
        }
        CHECK(rows == out[VS_O_ROWS] && (long long)seen.size() == out[VS_O_CONTIGS], "%s: counters", dst.c_str());
    }
    free(text);
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: tbi_check DIR [MORE.vcf ...]\n");
        return 2;
    }
    const std::string dir = argv[1];
    std::vector<std::string> names;
    DIR *d = opendir(dir.c_str());
    if (!d) {
        fprintf(stderr, "tbi_check: cannot list %s\n", dir.c_str());
        return 2;
    }
    while (struct dirent *e = readdir(d)) {
        const std::string nm = e->d_name;
        if (nm.size() > 4 && nm.compare(nm.size() - 4, 4, ".vcf") == 0) names.push_back(nm);
    }
    closedir(d);
    std::sort(names.begin(), names.end());
    for (const std::string &nm : names) one(dir + "/" + nm, dir + "/" + nm + ".gz", nm.compare(0, 8, "refused_") == 0);
    for (int i = 2; i < argc; i++) one(argv[i], dir + "/more" + std::to_string(i) + ".vcf.gz", false);
    if (fails) {
        fprintf(stderr, "tbi_check: %d failures\n", fails);
        return 1;
    }
    printf("tbi_check: ok (%zu files)\n", names.size() + (size_t)(argc - 2));
    return 0;
}
