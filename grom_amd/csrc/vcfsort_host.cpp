// vcfsort_host.cpp -- the host twin of the sorting, indexing VCF writer
// (DESIGN.md 4.9): vcfsort.hip's phases as loops over vcfsort.h's per-row
// arithmetic -- line starts, facts, contig runs, the stable LSD radix sort of
// (contig id << 32 | POS), the gather, the BGZF file through the compressor's
// host twin, the virtual offsets, bins, runs and linear windows -- and the
// host steps both paths share (names, messages, the .tbi, the renames).
// Plain C++, no HIP.  tests/test_vcf_tabix_host.py reads its files with an
// independent tabix reader; tools/tbi_check.cpp runs it under sanitizers; the
// GPU tests demand its bytes from the kernels.
#include "vcfsort_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <chrono>
#include <unordered_map>

#include "../../include/grom_amd.h"
#include "bamio.h"
#include "bgzfwrite.h"
#include "vcfsort.h"

const char *const VS_MSG_NO_NEWLINE = "VCF sort: the last line does not end in a newline";

void vs_refusal(int kind, int64_t line, char *err, size_t cap) {
    const char *what = kind == VS_E_HASH   ? "a '#' line after the first row"
                       : kind == VS_E_COLS ? "fewer than 8 columns"
                       : kind == VS_E_POS  ? "POS is not a decimal number"
                                           : "the row ends past 2^29: the .tbi index is limited to 512 Mb";
    snprintf(err, cap, "VCF sort: line %lld: %s", (long long)line, what);
}

// what is wrong with the line text[a, b) (VS_OK: a row, its facts in *f)
static int line_kind(const uint8_t *text, int64_t a, int64_t b, VsFacts *f) {
    if (text[a] == '#') return VS_E_HASH;
    return (*f = vs_facts(text, a, b)).err;
}

int vs_first_refusal(const uint8_t *text, int64_t n, char *err, size_t cap) {
    if (n > 0 && text[n - 1] != '\n') {
        snprintf(err, cap, "%s", VS_MSG_NO_NEWLINE);
        return 1;
    }
    int64_t line = 0, a = 0;
    bool rows = false;
    for (int64_t i = 0; i < n; i++) {
        if (text[i] != '\n') continue;
        line++;
        VsFacts f;
        if (rows || text[a] != '#') {
            rows = true;
            const int kind = line_kind(text, a, i + 1, &f);
            if (kind != VS_OK) {
                vs_refusal(kind, line, err, cap);
                return 1;
            }
        }
        a = i + 1;
    }
    return 0;
}

int32_t vs_map_names(const uint8_t *const *chunks, int64_t chunk, const int64_t *head, int64_t n_runs,
                     std::vector<uint32_t> &run_cid, std::string &names) {
    std::unordered_map<std::string, uint32_t> ids;
    run_cid.resize((size_t)n_runs);
    names.clear();
    std::string nm;
    for (int64_t r = 0; r < n_runs; r++) {
        nm.clear();
        for (int64_t e = head[r];; e++) {
            const uint8_t c = chunks[e / chunk][e % chunk];
            if (c == '\t' || c == '\n') break;
            nm.push_back((char)c);
        }
        auto it = ids.find(nm);
        if (it == ids.end()) {
            it = ids.emplace(nm, (uint32_t)ids.size()).first;
            names.append(nm);
            names.push_back('\0');
        }
        run_cid[(size_t)r] = it->second;
    }
    return (int32_t)ids.size();
}

int vs_passes(uint64_t diff, int digit[8]) {
    int n = 0;
    for (int d = 0; d < 8; d++)
        if ((diff >> (8 * d)) & 0xff) digit[n++] = d;
    return n;
}

static const uint8_t VS_EOF[28] = {0x1f, 0x8b, 0x08, 0x04, 0x00, 0x00, 0x00, 0x00, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43,
                                   0x02, 0x00, 0x1b, 0x00, 0x03, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00};

int vs_bgzf_file(const char *path, const uint8_t *data, int64_t n, const char *gzi_path, std::vector<int64_t> *coff) {
    FILE *fp = fopen(path, "wb");
    if (!fp) return -1;
    const int64_t n_blk = (n + VS_PAYLOAD - 1) / VS_PAYLOAD, BATCH = 64;
    std::vector<uint8_t> dst((size_t)(BATCH * (VS_PAYLOAD + 32) + 64));
    std::vector<int64_t> uo((size_t)BATCH + 1), co((size_t)BATCH + 1), all;
    int64_t at = 0;
    int rc = 0;
    for (int64_t b0 = 0; b0 < n_blk && rc == 0; b0 += BATCH) {
        const int64_t nb = n_blk - b0 < BATCH ? n_blk - b0 : BATCH;
        for (int64_t i = 0; i <= nb; i++) uo[(size_t)i] = (b0 + i) * VS_PAYLOAD < n ? (b0 + i) * VS_PAYLOAD : n;
        if (df_host_blocks(data, uo.data(), nb, dst.data(), (int64_t)dst.size(), co.data(), nullptr) != 0) rc = -1;
        for (int64_t i = 0; i < nb && rc == 0; i++) all.push_back(at + co[(size_t)i]);
        if (rc == 0 && fwrite(dst.data(), 1, (size_t)co[(size_t)nb], fp) != (size_t)co[(size_t)nb]) rc = -1;
        at += co[(size_t)nb];
    }
    all.push_back(at);  // the EOF marker's offset
    if (rc == 0 && fwrite(VS_EOF, 1, 28, fp) != 28) rc = -1;
    if (fclose(fp) != 0) rc = -1;
    if (rc == 0 && gzi_path) {
        // bgzip's .gzi: the count, then (compressed, uncompressed) of every block after the first
        FILE *g = fopen(gzi_path, "wb");
        const uint64_t cnt = n_blk > 1 ? (uint64_t)(n_blk - 1) : 0;
        if (!g || fwrite(&cnt, 8, 1, g) != 1) rc = -1;
        for (int64_t i = 1; i < n_blk && rc == 0; i++) {
            const uint64_t pr[2] = {(uint64_t)all[(size_t)i], (uint64_t)(i * VS_PAYLOAD)};
            if (fwrite(pr, 8, 2, g) != 2) rc = -1;
        }
        if (g && fclose(g) != 0) rc = -1;
    }
    if (coff) coff->swap(all);
    return rc;
}

int vs_write_tbi(const char *path, const std::string &names, int32_t n_ref, const VsRun *runs, int64_t n_runs,
                 const uint64_t *lin, const int64_t *lin_base, const VsSpan *span, int64_t counts[3], char *err,
                 size_t cap) {
    std::vector<bai_racc *> R((size_t)(n_ref > 0 ? n_ref : 1), nullptr);
    int rc = 0;
    for (int32_t c = 0; c < n_ref && rc == 0; c++)
        if (!(R[(size_t)c] = bai_racc_new())) rc = -1;
    for (int64_t r = 0; r < n_runs && rc == 0; r++) {
        if (runs[r].cid < 0 || runs[r].cid >= n_ref) { rc = -1; break; }
        bai_racc_add_run(R[(size_t)runs[r].cid], runs[r].bin, runs[r].beg, runs[r].end);
    }
    for (int32_t c = 0; c < n_ref && rc == 0; c++) {
        bai_racc_set_span(R[(size_t)c], span[c].beg, span[c].end, span[c].rows, 0);
        if (bai_racc_set_linear(R[(size_t)c], lin + lin_base[c], (int32_t)(lin_base[c + 1] - lin_base[c])) != 0) rc = -1;
    }
    char *mem = nullptr;
    size_t len = 0;
    counts[0] = counts[1] = counts[2] = 0;
    if (rc == 0) {
        FILE *f = open_memstream(&mem, &len);
        if (!f) rc = -1;
        else {
            if (tbi_write_racc(f, R.data(), n_ref, names.data(), (int32_t)names.size(), counts) != 0) rc = -1;
            if (fclose(f) != 0) rc = -1;
        }
    }
    for (bai_racc *a : R) bai_racc_free(a);
    if (rc == 0 && vs_bgzf_file(path, (const uint8_t *)mem, (int64_t)len, nullptr, nullptr) != 0) rc = -1;
    free(mem);
    if (rc) snprintf(err, cap, "VCF sort: cannot write the .tbi index %s", path);
    return rc;
}

int vs_commit(const std::string &path, const std::string &tmp_gz, const std::string &tmp_tbi, const std::string &tmp_gzi,
              bool ok, char *err, size_t cap) {
    if (ok) {
        if (rename(tmp_gz.c_str(), path.c_str()) == 0 && rename(tmp_tbi.c_str(), (path + ".tbi").c_str()) == 0 &&
            rename(tmp_gzi.c_str(), (path + ".gzi").c_str()) == 0)
            return 0;
        snprintf(err, cap, "VCF sort: cannot rename the files of %s", path.c_str());
        (void)remove(path.c_str());
        (void)remove((path + ".tbi").c_str());
        (void)remove((path + ".gzi").c_str());
    }
    (void)remove(tmp_gz.c_str());
    (void)remove(tmp_tbi.c_str());
    (void)remove(tmp_gzi.c_str());
    return -1;
}

int vs_host_run(const uint8_t *text, int64_t n, const char *path, int64_t out[12], char *err, size_t cap) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < 12; i++) out[i] = 0;
    if (n > 0 && text[n - 1] != '\n') {
        snprintf(err, cap, "%s", VS_MSG_NO_NEWLINE);
        return GROM_E_ARG;
    }
    // 1. lines
    std::vector<int64_t> ls;
    ls.push_back(0);
    for (int64_t i = 0; i < n; i++)
        if (text[i] == '\n') ls.push_back(i + 1);
    const int64_t L = (int64_t)ls.size() - 1;
    int64_t H = 0;
    while (H < L && text[ls[(size_t)H]] == '#') H++;
    const int64_t R = L - H;
    // 2. facts and contig runs
    std::vector<VsFacts> F((size_t)R);
    std::vector<int64_t> head;
    std::vector<uint32_t> run_of((size_t)R);
    for (int64_t i = 0; i < R; i++) {
        const int64_t a = ls[(size_t)(H + i)], b = ls[(size_t)(H + i + 1)];
        const int kind = line_kind(text, a, b, &F[(size_t)i]);
        if (kind != VS_OK) {
            vs_refusal(kind, H + i + 1, err, cap);
            return GROM_E_ARG;
        }
        if (i == 0 || !vs_same_chrom(text, ls[(size_t)(H + i - 1)], a, n)) head.push_back(a);
        run_of[(size_t)i] = (uint32_t)head.size() - 1;
    }
    std::vector<uint32_t> run_cid;
    std::string names;
    const int32_t C = vs_map_names(&text, INT64_MAX, head.data(), (int64_t)head.size(), run_cid, names);
    // 3. keys, the stable LSD radix sort
    std::vector<uint64_t> key((size_t)R), key2((size_t)R);
    std::vector<uint32_t> idx((size_t)R), idx2((size_t)R);
    uint64_t diff = 0;
    int64_t inv = 0;
    for (int64_t i = 0; i < R; i++) {
        key[(size_t)i] = vs_key(run_cid[run_of[(size_t)i]], F[(size_t)i].pos);
        idx[(size_t)i] = (uint32_t)i;
        diff |= key[(size_t)i] ^ key[0];
        if (i > 0 && key[(size_t)i] < key[(size_t)i - 1]) inv++;
    }
    int digit[8];
    const int np = vs_passes(diff, digit);
    for (int k = 0; k < np; k++) {
        const int sh = 8 * digit[k];
        int64_t cnt[257] = {0};
        for (int64_t i = 0; i < R; i++) cnt[((key[(size_t)i] >> sh) & 0xff) + 1]++;
        for (int d = 0; d < 256; d++) cnt[d + 1] += cnt[d];
        for (int64_t i = 0; i < R; i++) {
            const int64_t at = cnt[(key[(size_t)i] >> sh) & 0xff]++;
            key2[(size_t)at] = key[(size_t)i];
            idx2[(size_t)at] = idx[(size_t)i];
        }
        key.swap(key2);
        idx.swap(idx2);
    }
    // 4. gather
    const int64_t hb = ls[(size_t)H];
    std::vector<uint8_t> sorted((size_t)n + 1);
    std::vector<int64_t> doff((size_t)R + 1);
    if (hb) memcpy(sorted.data(), text, (size_t)hb);
    int64_t at = hb;
    for (int64_t j = 0; j < R; j++) {
        const int64_t a = ls[(size_t)(H + idx[(size_t)j])], len = ls[(size_t)(H + idx[(size_t)j] + 1)] - a;
        doff[(size_t)j] = at;
        memcpy(sorted.data() + at, text + a, (size_t)len);
        at += len;
    }
    doff[(size_t)R] = at;
    const std::string tag = ".tmp." + std::to_string((long long)getpid());
    const std::string p = path, tmp_gz = p + tag, tmp_tbi = p + ".tbi" + tag, tmp_gzi = p + ".gzi" + tag;
    std::vector<int64_t> coff;
    if (vs_bgzf_file(tmp_gz.c_str(), sorted.data(), n, tmp_gzi.c_str(), &coff) != 0) {
        snprintf(err, cap, "VCF sort: cannot write %s", path);
        vs_commit(p, tmp_gz, tmp_tbi, tmp_gzi, false, err, cap);
        return GROM_E_ARG;
    }
    // 5. index
    const int64_t n_blk = (int64_t)coff.size() - 1;
    std::vector<VsRun> runs;
    std::vector<VsSpan> span((size_t)C + 1);
    std::vector<int64_t> lin_base((size_t)C + 2, 0);
    {
        std::vector<int32_t> maxw((size_t)C + 1, 0);
        for (int64_t j = 0; j < R; j++) {
            const uint32_t c = (uint32_t)(key[(size_t)j] >> 32);
            const int32_t w = ((F[idx[(size_t)j]].end0 - 1) >> 14) + 1;
            if (w > maxw[c]) maxw[c] = w;
        }
        for (int32_t c = 0; c < C; c++) lin_base[(size_t)c + 1] = lin_base[(size_t)c] + maxw[(size_t)c];
    }
    std::vector<uint64_t> lin((size_t)lin_base[(size_t)C] + 1, VS_NONE);
    for (int64_t j = 0; j < R; j++) {
        const VsFacts &f = F[idx[(size_t)j]];
        const int32_t c = (int32_t)(key[(size_t)j] >> 32);
        const uint32_t bin = vs_reg2bin(f.beg0, f.end0);
        const uint64_t vb = vs_voff(coff.data(), n_blk, n, doff[(size_t)j]), ve = vs_voff(coff.data(), n_blk, n, doff[(size_t)j + 1]);
        if (runs.empty() || runs.back().cid != c || runs.back().bin != bin) runs.push_back(VsRun{c, bin, vb, ve});
        runs.back().end = ve;
        for (int32_t w = f.beg0 >> 14; w <= (f.end0 - 1) >> 14; w++) {
            uint64_t &l = lin[(size_t)(lin_base[(size_t)c] + w)];
            if (vb < l) l = vb;
        }
        VsSpan &s = span[(size_t)c];
        if (s.rows == 0) s.beg = vb;
        s.end = ve;
        s.rows++;
    }
    int64_t counts[3];
    const bool ok = vs_write_tbi(tmp_tbi.c_str(), names, C, runs.data(), (int64_t)runs.size(), lin.data(), lin_base.data(),
                                 span.data(), counts, err, cap) == 0;
    if (vs_commit(p, tmp_gz, tmp_tbi, tmp_gzi, ok, err, cap) != 0) return GROM_E_ARG;
    out[VS_O_ROWS] = R;
    out[VS_O_HEADER] = H;
    out[VS_O_CONTIGS] = C;
    out[VS_O_INVERSIONS] = inv;
    out[VS_O_PASSES] = np;
    out[VS_O_BINS] = counts[0];
    out[VS_O_CHUNKS] = counts[1];
    out[VS_O_WINDOWS] = counts[2];
    out[VS_O_US_WALL] = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}
