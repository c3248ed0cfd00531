/* ctxpost.c -- main's translocation post-pass (GROM.c:22400-22770), pure host
 * arithmetic: the raw CTX rows of every chromosome are read back, each
 * breakpoint is paired with a mate row (its chromosome and mate chromosome
 * swapped, positions within insert_max - 2*lseq, orientations consistent), the
 * weaker of two nearby paired rows is dropped with its mate, and the rest are
 * written as BND rows. */
#include <ctype.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/grom_amd.h"
#include "ctxpost.h"

typedef struct {
    int type, chr, pos, rd, conc, other, mchr, mpos, rs, re, mateid, keep;
    double binom, ev, hez;
} ctx_row_t;

void ctx_postpass(const char *raw, size_t raw_len, const bam_hdr *hdr, int Mx, int glseq, int vcf, FILE *out) {
    int n_t = hdr->n_ref;
    char **lc = calloc(n_t > 0 ? n_t : 1, sizeof(char *));
    for (int a = 0; a < n_t; a++) {
        size_t L = strlen(hdr->ref_name[a]);
        lc[a] = malloc(L + 1);
        for (size_t b = 0; b <= L; b++) lc[a][b] = (char)tolower((unsigned char)hdr->ref_name[a][b]);
    }
    int n = 0, cap = 1024;
    ctx_row_t *rw = calloc(cap, sizeof(ctx_row_t));
    size_t off = 0;
    while (raw && off < raw_len) {
        const char *e = memchr(raw + off, '\n', raw_len - off);
        size_t ll = e ? (size_t)(e - (raw + off)) : raw_len - off;
        char *line = malloc(ll + 1);
        memcpy(line, raw + off, ll);
        line[ll] = 0;
        off += ll + (e ? 1 : 0);
        if (n == cap) { cap *= 2; rw = realloc(rw, cap * sizeof(ctx_row_t)); }
        ctx_row_t *q = &rw[n++];
        memset(q, 0, sizeof(*q));
        char *save = NULL, *t = strtok_r(line, "\t", &save);
        q->type = t ? (strcmp(t, "CTX_F") == 0 ? 6 : strcmp(t, "CTX_R") == 0 ? 7 : -1) : -1; /* g_sv_types */
        t = strtok_r(NULL, "\t", &save);
        q->chr = -1;
        if (t) {
            char tl[1024];
            size_t L = strlen(t);
            if (L > sizeof(tl) - 1) L = sizeof(tl) - 1;
            for (size_t b = 0; b < L; b++) tl[b] = (char)tolower((unsigned char)t[b]);
            tl[L] = 0;
            for (int a = 0; a < n_t; a++)
                if (strcmp(lc[a], tl) == 0) { q->chr = a; break; }
        }
        int *ifld[] = {&q->pos, NULL, NULL, &q->rd, &q->conc, &q->other, &q->mchr, &q->mpos, &q->rs, &q->re, NULL};
        double *dfld[] = {NULL, &q->binom, &q->ev, NULL, NULL, NULL, NULL, NULL, NULL, NULL, &q->hez};
        for (int k = 0; k < 11; k++) {
            t = strtok_r(NULL, "\t", &save);
            if (ifld[k]) *ifld[k] = t ? atoi(t) : 0;
            else *dfld[k] = t ? atof(t) : 0;
        }
        free(line);
    }
    const int span = Mx - 2 * glseq;
    for (int b = 0; b < n; b++) { rw[b].keep = 0; rw[b].mateid = -1; }
    for (int b = 0; b < n; b++)
        for (int c = 0; c < n; c++) {
            if (!(rw[b].chr == rw[c].mchr && rw[c].chr == rw[b].mchr)) continue;
            if (!(abs(rw[b].pos - abs(rw[c].mpos)) < span && abs(rw[c].pos - abs(rw[b].mpos)) < span)) continue;
            const int bo = (rw[b].type == 6 && rw[c].mpos >= 0) || (rw[b].type == 7 && rw[c].mpos < 0);
            const int co = (rw[c].type == 6 && rw[b].mpos >= 0) || (rw[c].type == 7 && rw[b].mpos < 0);
            if (bo && co) {
                rw[b].keep = 1;
                rw[b].mateid = c;
                rw[b].mpos = rw[b].mpos < 0 ? -rw[c].pos : rw[c].pos;
            }
        }
    for (int b = 0; b < n; b++)
        for (int c = 0; c < n; c++) {
            if (b == c || rw[b].chr != rw[c].chr || rw[b].mchr != rw[c].mchr) continue;
            if (!(abs(rw[b].pos - rw[c].pos) < span && abs(abs(rw[b].mpos) - abs(rw[c].mpos)) < span)) continue;
            if (rw[b].keep == 1 && rw[c].keep == 1 && (rw[b].binom > rw[c].binom || (rw[b].binom == rw[c].binom && b > c))) {
                rw[b].keep = 0;
                if (rw[b].mateid >= 0) rw[rw[b].mateid].keep = 0;
            }
        }
    printf("Translocations before filter: %d\n", n);
    int n2 = 0;
    for (int b = 0; b < n; b++) {
        const ctx_row_t *q = &rw[b];
        if (q->keep != 1) continue;
        n2++;
        char bnd[64];
        const char *mn = (q->mchr >= 0 && q->mchr < n_t) ? lc[q->mchr] : "";
        if (!vcf) { /* -f rows, GROM.c:22734 (g_sv_types[6] "CTX_F", [7] "CTX_R", GROM.c:867) */
            fprintf(out, "%s\t%s\t%d\t%d\t%d\t%e\t%.1f\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%e\n", q->type == 6 ? "CTX_F" : "CTX_R",
                    (q->chr >= 0 && q->chr < n_t) ? lc[q->chr] : "", q->pos, b, q->mateid, q->binom, q->ev, q->rd, q->conc,
                    q->other, mn, q->mpos, q->rs, q->re, q->hez);
            continue;
        }
        const int am = abs(q->mpos);
        if (q->type == 6) snprintf(bnd, sizeof(bnd), q->mpos < 0 ? "N[%s:%d[" : "N]%s:%d]", mn, am);
        else snprintf(bnd, sizeof(bnd), q->mpos < 0 ? "[%s:%d[N" : "]%s:%d]N", mn, am);
        fprintf(out, "%s\t%d\t%d\tN\t%s\t.\t.\tSVTYPE=BND;MATEID=%d\tSPR:SEV:SRD:SCO:SOT:SFR:SLR:SHPR\t%e:%.1f:%d:%d:%d:%d:%d:%e\n",
                (q->chr >= 0 && q->chr < n_t) ? lc[q->chr] : "", q->pos + 1, b, bnd, q->mateid, q->binom, q->ev, q->rd,
                q->conc, q->other, q->rs + 1, q->re + 1, q->hez);
    }
    printf("Translocations after filter: %d\n", n2);
    for (int a = 0; a < n_t; a++) free(lc[a]);
    free(lc);
    free(rw);
}

int grom_ctx_postpass(const char *raw, size_t raw_len, const char *const *target_names, int32_t n_targets,
                      int32_t insert_max, int32_t lseq, grom_out *out) {
    if (!out || n_targets < 0 || (n_targets > 0 && !target_names)) {
        grom_set_last_error("grom_ctx_postpass: bad argument");
        return GROM_E_ARG;
    }
    bam_hdr h;
    memset(&h, 0, sizeof(h));
    h.n_ref = n_targets;
    h.ref_name = (char **)target_names;
    char *buf = NULL;
    size_t len = 0;
    FILE *f = open_memstream(&buf, &len);
    if (!f) { grom_set_last_error("grom_ctx_postpass: no memory"); return GROM_E_NOMEM; }
    ctx_postpass(raw, raw_len, &h, insert_max, lseq, 1, f);
    fclose(f);
    if (out->ctx_len + len + 1 > out->ctx_cap) {
        size_t nc = out->ctx_cap ? out->ctx_cap : 4096;
        while (nc < out->ctx_len + len + 1) nc *= 2;
        char *p = realloc(out->ctx, nc);
        if (!p) { free(buf); grom_set_last_error("grom_ctx_postpass: no memory"); return GROM_E_NOMEM; }
        out->ctx = p;
        out->ctx_cap = nc;
    }
    memcpy(out->ctx + out->ctx_len, buf, len);
    out->ctx_len += len;
    out->ctx[out->ctx_len] = 0;
    free(buf);
    return GROM_OK;
}
