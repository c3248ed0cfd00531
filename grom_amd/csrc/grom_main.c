/*
 * grom_main.c -- `grom`, the drop-in command line for GROM's scan.
 *
 * Mirrors GROM's main (GROM.c:21865-22781) and find_disc_svs
 * (GROM.c:20440-21129): the same getopt string and defaults, the same output
 * files (OUT and OUT's .ctx.vcf sibling), the same chromosome selection and
 * order.  The per-chromosome scan (count_discordant_pairs, GROM.c:1432) runs
 * on the GPU through include/grom_amd.h.
 *
 * Options that steer parts of the reference outside the implemented scan rows
 * are accepted and recorded.  The GROM_* environment knobs are read once per
 * run (cli_settings.c lists them); the translocation post-pass is ctxpost.c.
 */
#define _GNU_SOURCE /* fopencookie: the rows' FILE over the BGZF writer (GROM_VCF_BGZF) */
#include <dirent.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <execinfo.h>
#include <signal.h>
#include <time.h>
#include <unistd.h>
#include <sys/mman.h>

#include "../../include/grom_amd.h"
#include "bamio.h"
#include "cli_settings.h"
#include "ctxpost.h"
#include "ddecode.h"
#include "stream.h"
#include "pdecode.h"

static const char *VERSION = "GROM, Version 1.0.1\n"; /* g_version_name, GROM.c:690 */

static void print_help(void) {
    /* GROM.c:1125-1181 */
    printf("\n%s", VERSION);
    printf("\nUsage: GROM -i <BAM input file> -r <REFERENCE input file> -o <output file> [optional parameters]\n");
    printf("\nRequired Parameters:\n");
    printf("\t-i \tBAM input file\n");
    printf("\t-r \tREFERENCE input file (fasta)\n");
    printf("\t-o \tSTRUCTURAL VARIANT output file\n");
    printf("\nOptional Parameters:\n");
    printf("\t-P \tthreads [1]\n");
    printf("\t-M \tturn on GROM's duplicate read filtering\n");
    printf("\t-q \tmapping quality threshold [35]\n");
    printf("\t-s \tminimum standard deviations for discordance [3]\n");
    printf("\t-v \tprobability threshold [0.001]\n");
    printf("\t-g \tgender (0=female,1=male) [0]\n");
    printf("\t-d \tminimum discordant pairs [3]\n");
    printf("\t-b \tbase phred quality score threshold [35]\n");
    printf("\t-n \tminimum SNV bases [3]\n");
    printf("\t-a \tminimum SNV ratio [0.2]\n");
    printf("\t-y \tmaximum unmapped gap or overlap for split reads [20]\n");
    printf("\t-z \tminimum split read mapped length (each split) [30]\n");
    printf("\t-S \tturn off split-read detection\n");
    printf("\t-p \tploidy [2]\n");
    printf("\t-e \tinsertion probability threshold [0.0000000001]\n");
    printf("\t-j \tminimum SV ratio [0.05]\n");
    printf("\t-k \tmaximum homopolymer (indels) [0.05]\n");
    printf("\t-m \tminimum indel ratio [0.125]\n");
    printf("\t-u \tmaximum evidence ratio (SV except insertion) [0.25]\n");
    printf("\t-A \tsampling rate [2]\n");
    printf("\t-V \tread depth p-value threshold [0.000001]\n");
    printf("\t-W \twindow minimum size [100]\n");
    printf("\t-X \twindow maximum size [10000]\n");
    printf("\t-Y \tminimum number of blocks [4]\n");
    printf("\t-Z \tblock minimum size [10000]\n");
    printf("\t-U \texcessive coverage threshold [2]\n");
    printf("\t-B \tchromosome maximum length [300000000]\n");
    printf("\t-D \tdinucleotide repeat minimum length [20]\n");
    printf("\t-E \tdinucleotide repeat minimum standard deviation [1.5]\n");
    printf("\t-K \tranks (0=no ranking,1=use ranks) [1]\n");
    printf("\t-L \tduplication coverage threshold [2]\n");
    printf("\nSee README file for additional help.\n");
    printf("\n");
}

static void header(FILE *f, const char *fasta_name, int ctx, const char *pin) {
    /* GROM.c:20517-20565 (main VCF) and GROM.c:22612-22651 (.ctx.vcf); `pin`: GROM_FILEDATE */
    fprintf(f, "##fileformat=VCFv4.2\n");
    if (pin) {
        fprintf(f, "##fileDate=%s\n", pin);
    } else {
        time_t t = time(NULL);
        struct tm tm = *localtime(&t);
        fprintf(f, "##fileDate=%d%d%d\n", tm.tm_year + 1900, tm.tm_mon + 1, tm.tm_mday);
    }
    fprintf(f, "##reference=%s\n", fasta_name);
    fprintf(f, "##ALT=<ID=DEL,Description=\"Deletion\">\n");
    fprintf(f, "##ALT=<ID=DUP,Description=\"Duplication\">\n");
    fprintf(f, "##ALT=<ID=INS,Description=\"Insertion\">\n");
    fprintf(f, "##ALT=<ID=INV,Description=\"Inversion\">\n");
    fprintf(f, "##INFO=<ID=END,Number=1,Type=Integer,Description=\"End position of the structural variant\">\n");
    if (!ctx) fprintf(f, "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n");
    static const char *fmt_lines[][2] = {
        {"SPR", "Float,Description=\"Probability of start breakpoint evidence occurring by chance"},
        {"EPR", "Float,Description=\"Probability of end breakpoint evidence occurring by chance"},
        {"SEV", "Integer,Description=\"Evidence supporting variant at start breakpoint"},
        {"EEV", "Integer,Description=\"Evidence supporting variant at end breakpoint"},
        {"SRD", "Integer,Description=\"Physical read depth at start breakpoint"},
        {"ERD", "Integer,Description=\"Physical read depth at end breakpoint"},
        {"SCO", "Integer,Description=\"Concordant pairs at start breakpoint"},
        {"ECO", "Integer,Description=\"Concordant pairs at end breakpoint"},
        {"SOT", "Integer,Description=\"Count of distinct SVs with evidence at start breakpoint"},
        {"EOT", "Integer,Description=\"Count of distinct SVs with evidence at end breakpoint"},
        {"SSC", "Integer,Description=\"Soft-clipped reads at start breakpoint"},
        {"ESC", "Integer,Description=\"Soft-clipped at end breakpoint"},
        {"SFR", "Integer,Description=\"Position of first read supporting start breakpoint"},
        {"SLR", "Integer,Description=\"Position of last read supporting start breakpoint"},
        {"EFR", "Integer,Description=\"Position of first read supporting end breakpoint"},
        {"ELR", "Integer,Description=\"Position of last read supporting end breakpoint"},
        {"AF", "Float,Description=\"Allele frequency (high mapping quality reads)"},
        {"PR", "Float,Description=\"Probability of SNV evidence occurring by chance"},
        {"A", "Integer,Description=\"A nucleotides (high mapping quality reads)"},
        {"C", "Integer,Description=\"C nucleotides (high mapping quality reads)"},
        {"G", "Integer,Description=\"G nucleotides (high mapping quality reads)"},
        {"T", "Integer,Description=\"T nucleotides (high mapping quality reads)"},
        {"AL", "Integer,Description=\"A nucleotides (low mapping quality reads)"},
        {"CL", "Integer,Description=\"C nucleotides (low mapping quality reads)"},
        {"GL", "Integer,Description=\"G nucleotides (low mapping quality reads)"},
        {"TL", "Integer,Description=\"T nucleotides (low mapping quality reads)"},
        {"BQ", "Float,Description=\"Average base quality (all reads)"},
        {"MQ", "Float,Description=\"Average mapping quality (all reads)"},
        {"PIR", "Float,Description=\"Average distance of SNV from DNA fragment end)"},
        {"FS", "Integer,Description=\"SNV reads mapped to forward strand)"},
    };
    for (size_t i = 0; i < sizeof(fmt_lines) / sizeof(fmt_lines[0]); i++)
        fprintf(f, "##FORMAT=<ID=%s,Number=1,Type=%s\">\n", fmt_lines[i][0], fmt_lines[i][1]);
    if (!ctx) {
        fprintf(f, "##FORMAT=<ID=SD,Number=1,Type=Float,Description=\"CNV standard deviation\"\n");
        fprintf(f, "##FORMAT=<ID=Z,Number=1,Type=Float,Description=\"CNV probability score\"\n");
        fprintf(f, "##FORMAT=<ID=CN,Number=1,Type=Float,Description=\"CNV copy number\"\n");
        fprintf(f, "##FORMAT=<ID=CS,Number=1,Type=Float,Description=\"CNV copy number standard deviation\"\n");
    }
    fprintf(f, "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\n");
}

/* -f: the insert statistics and the column header instead of the VCF header
 * (GROM.c:20566-20671) */
static const char TAB_COLUMNS[] =
    "SV\tChromosome\tStart (Tumor)\tEnd (Tumor)\tLength (Tumor)\tP-val (Start, Tumor)\t"
    "P-val (End, Tumor)\tConcordant Pairs (Start, Tumor)\tConcordant Pairs (End, Tumor)\t"
    "Start or End?\tRead Depth (High MapQ, Normal)\tRead Depth (Low MapQ, Normal)\t"
    "Concordant Pairs (Normal)\tINS (Normal)\tDEL (For, Normal)\tDEL (Rev, Normal)\t"
    "DEL (For, Length, Normal)\tDEL (Rev, Length, Normal)\tDUP (Rev, Normal)\tDUP (For, Normal)\t"
    "DUP (Rev, Length, Normal)\tDUP (For, Length, Normal)\tINV (For, Start, Normal)\t"
    "INV (Rev, Start, Normal)\tINV (For, End, Normal)\tINV (Rev, End, Normal)\t"
    "INV (For, Start, Length, Normal)\tINV (Rev, Start, Length, Normal)\t"
    "INV (For, End, Length, Normal)\tINV (Rev, End, Length, Normal)\tUnmapped Mate (For, Normal)\t"
    "Unmapped Mate (Rev, Normal)\tSoft-clipping (Left, Normal)\tSoft-clipping (Right, Normal)\t"
    "Soft-clipping Read Depth (Left, Normal)\tSoft-clipping Read Depth (Right, Normal)\t"
    "Soft-clipping Read Depth (Left+Right, Normal)\tINS Indel (Normal)\tDEL Indel (Start, Normal)\t"
    "DEL Indel (End, Normal)\tDEL Indel (Start, Length, Normal)\tDEL Indel (End, Length, Normal)\t"
    "CTX Soft-clipping (Left, Normal)\tCTX Soft-clipping (Right, Normal)\t"
    "CTX Soft-clipping Read Depth (Left, Normal)\tCTX Soft-clipping Read Depth (Right, Normal)\t"
    "CTX Soft-clipping Read Depth (Left+Right, Normal)\tIndel Soft-clipping (Left, Normal)\t"
    "Indel Soft-clipping (Right, Normal)\tIndel Soft-clipping Read Depth (Left, Normal)\t"
    "Indel Soft-clipping Read Depth (Right, Normal)\t"
    "Indel Soft-clipping Read Depth (Left+Right, Normal)\t"
    "Soft-clipping (Left Max including CTX, Normal)\t"
    "Soft-clipping (Right Max including CTX, Normal)\tOther (Number of Non-Empty, Normal)\t"
    "CTX (For, Normal)\tCTX (Rev, Normal)\tSV Overlap (Normal)\tOther (Number of Non-Empty, Tumor)\t"
    "Read Start (Start, Tumor)\tRead End (Start, Tumor)\tRead Start (End, Tumor)\t"
    "Read End (End, Tumor)\tDEL Read Start (For/Rev, Normal)\tDEL Read End (For/Rev, Normal)\t"
    "DUP Read Start (Rev/For, Normal)\tDUP Read End (Rev/For, Normal)\tINV Read Start (For, Normal)\t"
    "INV Read End (For, Normal)\tINV Read Start (Rev, Normal)\tINV Read End (Rev, Normal)\t"
    "CTX Read Start (For, Normal)\tCTX Read End (For, Normal)\tCTX Read Start (Rev, Normal)\t"
    "CTX Read End (Rev, Normal)\tMate Chr (CTX only, Tumor)\tMate Pos (CTX only, Tumor)\t"
    "Mate Chr (For, Normal)\tMate Pos (For, Normal)\tMate Chr (Rev, Normal)\tMate Pos (Rev, Normal)\t"
    "Reference Base\tSNV Base (Tumor)\tSNV Ratio (Tumor)\tSNV Count (A, Tumor)\t"
    "SNV Count (C, Tumor)\tSNV Count (G, Tumor)\tSNV Count (T, Tumor)\tSNV Count (A, Normal)\t"
    "SNV Count (C, Normal)\tSNV Count (G, Normal)\tSNV Count (T, Normal)\t\n";
static void tab_header(FILE *f, const grom_params *P) {
    fprintf(f, "%d\t%d\t%d\t%d\n", P->insert_mean, P->insert_min_size, P->insert_max_size, P->lseq);
    fputs(TAB_COLUMNS, f);
}

typedef struct {
    int fasta_idx;
    int32_t tid;
    char *ref;
    const void *d_ref; /* the same bytes in device memory (the device FASTA loader's), else NULL */
    long len;
    char name[GROM_MAX_CHR_NAME_LEN + 1];
    char *target; /* BAM name the SA/XP chromosome test compares with (GROM.c:1894-1961, 7431) */
} chrom_plan;

static double clock_gettime_s(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

/* seconds from this process's start (the kernel's start time, clock ticks
 * since boot) to now: what loading the program and the library took before
 * the CLI's first line; -1 when /proc does not say */
static double since_process_start(void) {
    FILE *f = fopen("/proc/self/stat", "r");
    if (!f) return -1.0;
    char buf[2048];
    const size_t n = fread(buf, 1, sizeof(buf) - 1, f);
    fclose(f);
    buf[n] = 0;
    const char *p = strrchr(buf, ')'); /* (the command name may hold spaces) */
    if (!p) return -1.0;
    unsigned long long start = 0;
    int field = 2;
    for (const char *q = p + 1; *q && field < 22; q++)
        if (*q == ' ') {
            field++;
            if (field == 22) start = strtoull(q + 1, NULL, 10);
        }
    struct timespec t;
    clock_gettime(CLOCK_BOOTTIME, &t);
    const long hz = sysconf(_SC_CLK_TCK);
    if (start == 0 || hz <= 0) return -1.0;
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec - (double)start / (double)hz;
}

typedef struct {
    char *p;
    size_t len, cap;
} textbuf;

static void textbuf_add(textbuf *t, const char *s, size_t n) {
    if (t->len + n + 1 > t->cap) {
        size_t nc = t->cap ? 2 * t->cap : 1 << 16;
        while (nc < t->len + n + 1) nc *= 2;
        t->p = realloc(t->p, nc);
        t->cap = nc;
    }
    memcpy(t->p + t->len, s, n);
    t->len += n;
    t->p[t->len] = 0;
}

/* one run's state: everything the two input paths share */
typedef struct {
    grom_params P;
    cli_settings env; /* the GROM_* knobs, read at the run's start */
    /* grom_cli_main's flag, which outlives a run's second attempt: set once
     * the streamed run printed the insert lines, so that the serial rerun
     * after a late fallback (the index plan contradicted mid-file) does not
     * print them again and stdout reads as one run */
    int *insert_printed;
    const char *bam_name, *fasta_name, *out_name;
    const char *side_base; /* -o name: the -N side files are named after it */
    long max_chr_len;
    double num_sd;
    int device, force_serial;
    /* the device plan (plan_devices) */
    int n_dev;                        /* GPUs, from `device` on */
    int wdev[CLI_MAX_WORKERS], n_work; /* scan worker -> GPU */
    int n_init;                       /* library contexts made */
    bam_hdr hdr;
    grom_fasta fa;
    /* the device FASTA loader (fastadev.hip) of this run: a BGZF -r by
     * default, a plain one with GROM_FASTA_DEVICE=1.  One thread at a time
     * uses the handle */
    grom_fasta_dev *fdev;
    pthread_mutex_t fdev_mu;
    double *hez, *mq;
    pthread_t tables_thr;
    int tables_started;
    chrom_plan *plan; /* candidates in BAM order (preliminary: before the length test) */
    int n_cand;
    char ctx_name[4096];
    /* GROM_VCF_SEGS (a multi-GPU rank's run): where each chromosome's rows lie
     * in the VCF, "chromosome<TAB>offset<TAB>bytes" per line, so a merge of
     * the ranks' files copies byte ranges without reading the rows
     * (grom_amd.shard.merge_rank_outputs_parallel) */
    textbuf vcf_segs;
    double t_cli0, t_cand; /* CLI start, candidates (FASTA lengths) done */
    double t_load;         /* process start to the CLI's start (program and library loading) */
    double t_scans, t_pdclose, t_outputs; /* scans done, decoder closed, outputs written */
    double t_decclose;                     /* the decoder's host side closed */
    pthread_t hip_thr;     /* HIP runtime start-up, beside the header/FASTA/index work */
    int hip_started, hip_done;
    /* -P n (1..256, GROM.c:21923-21927): every chromosome reads its own
     * target's records (bam_fetch, GROM.c:21051-21064 and the -c children of
     * GROM.c:549-599) -- pd_set_fetch_mode; GROM_P_SERIAL=1 keeps the serial
     * stream's input (a one-process run's rows) on n GPUs */
    int fetch;
    /* -c chr,sub,start,end (GROM.c:21928-21930): one child of a -P n run --
     * BAM target `one_chrom` alone, read through bam_fetch, its rows to
     * OUT.<target>-<sub> and its raw CTX rows to OUT.<target>-<sub>.ctx, no
     * header, no translocation post-pass (the parent concatenates and pairs,
     * GROM.c:603-624, 22400), the insert statistics from <bam>.mean
     * (GROM.c:22253-22257).  Whole chromosomes only (start 0, end at or past
     * the chromosome's end: the children -P n forks without -R). */
    int one_chrom, sub_child, sub_start, sub_end;
    char part_name[4096];
    /* GROM_VCF_BGZF: the rows and the CTX file go out as BGZF (<name>.gz),
     * compressed on the run's first device; what each close reported
     * (GROM_VCF_TABIX: through the sorting, indexing writer, out[12]) */
    char gz_name[4100], ctx_gz_name[4100];
    int64_t gz_rows[12], gz_ctx[12];
    int gz_failed;
} cli_state;

static void plan_release_dref(cli_state *S, chrom_plan *c) {
    if (!c->d_ref) return;
    pthread_mutex_lock(&S->fdev_mu);
    if (S->fdev) grom_fasta_dev_release(S->fdev, c->d_ref);
    c->d_ref = NULL;
    pthread_mutex_unlock(&S->fdev_mu);
}

/* ---- one chromosome's scan, from either input path ----
 * serial path: `batch` holds the chromosome's records in host memory;
 * streamed path: `stage` holds them in HBM (pdecode.c) and `facts` the
 * serial stream's facts about them. */
typedef struct {
    chrom_plan *cp;
    grom_batch batch;
    int has_batch;
    grom_stage *stage;
    pd_chrom_facts facts;
    pd_session *pd;        /* releases the stage after the scan */
    int stage_released;    /* the scan gave the stage back before its CNV path */
    int k;                 /* plan index (trace) */
    int device;            /* the GPU the stage lives on, -1: any */
    char *text, *ctx_text;
    size_t text_len, ctx_len;
    int rc, ready, done, taken;
    char err[512];
} grom_job;

static void dump_file(const char *dump, const char *chr, const char *ext, const void *p, size_t bytes) {
    char path[4096];
    snprintf(path, sizeof(path), "%s.%s.%s", dump, chr, ext);
    FILE *f = fopen(path, "wb");
    if (!f) return;
    if (bytes) fwrite(p, 1, bytes, f);
    fclose(f);
}

static void write_dumps(const char *dump, int slot, const chrom_plan *cp, const grom_chrom *ch,
                        const grom_reads *host_rd, grom_stage *stage, const grom_params *P) {
    /* test hook (GROM_DUMP): per-base counters and caf depth, same files as the oracle's */
    int32_t first = 0;
    int32_t lo = P->one_base_rd_len / 4 + 1;
    if (lo < 2 * P->insert_max_size + 1) lo = 2 * P->insert_max_size + 1;
    int64_t n_eval = (ch->p_last >= lo) ? (int64_t)ch->p_last - lo + 1 : 0;
    int32_t *cnt = malloc(sizeof(int32_t) * GROM_NCOUNT * (n_eval > 0 ? n_eval : 1));
    int32_t *caf = malloc(sizeof(int32_t) * 3 * cp->len);
    int rc = stage ? grom_debug_counts_staged(slot, stage, ch, &first, cnt, GROM_NCOUNT * n_eval, caf)
                   : grom_debug_counts(slot, ch, host_rd, &first, cnt, GROM_NCOUNT * n_eval, caf);
    if (rc == GROM_OK) {
        dump_file(dump, cp->name, "cnt", cnt, sizeof(int32_t) * GROM_NCOUNT * (size_t)n_eval);
        dump_file(dump, cp->name, "caf", caf, sizeof(int32_t) * 3 * (size_t)cp->len);
        /* indel evidence of the same scan (row A7) */
        int64_t n_ind = grom_debug_indels(slot, NULL, 0);
        grom_indel_rec *ind = n_ind > 0 ? malloc(sizeof(grom_indel_rec) * n_ind) : NULL;
        if (n_ind >= 0 && (n_ind == 0 || (ind && grom_debug_indels(slot, ind, n_ind) == n_ind))) {
            dump_file(dump, cp->name, "ind", ind, sizeof(grom_indel_rec) * (size_t)n_ind);
        } else {
            fprintf(stderr, "grom: indel dump of %s failed: %s\n", cp->name, grom_last_error());
        }
        free(ind);
        /* breakpoint cluster records (rows A8/A9; the scan keeps them when
         * GROM_SV_DEBUG is set) */
        int64_t n_sv = grom_debug_sv(slot, NULL, 0);
        grom_sv_rec *svr = n_sv > 0 ? malloc(sizeof(grom_sv_rec) * n_sv) : NULL;
        if (n_sv >= 0 && (n_sv == 0 || (svr && grom_debug_sv(slot, svr, n_sv) == n_sv)))
            dump_file(dump, cp->name, "sv", svr, sizeof(grom_sv_rec) * (size_t)n_sv);
        free(svr);
    } else {
        fprintf(stderr, "grom: counter dump of %s failed: %s\n", cp->name, grom_last_error());
    }
    free(cnt);
    free(caf);
}

/* GROM_CHROMS=name[,name...]: scan and write only these chromosomes (one
 * rank's share of a genome, bench.py --gpus N); the others keep their place
 * in the plan, so each scanned chromosome gets the records the serial stream
 * of a whole run would give it */
static int chrom_wanted(const cli_state *S, const char *name) {
    const char *w = S->env.chroms;
    const size_t L = strlen(name);
    if (!w || !*w) return 1;
    for (const char *p = w; L && (p = strstr(p, name)) != NULL; p++) /* a whole entry of the list? */
        if ((p == w || p[-1] == ',') && (p[L] == ',' || !p[L])) return 1;
    return 0;
}

/* test hook (GROM_STAGE_DIGEST): the staged input of a chromosome, copied
 * back to the host, as the plan-only line prints it (the device decoder's
 * output against the host decoder's, tests/test_gpu_parity.py) */
static void stage_digest_line(grom_stage *st, const grom_chrom *ch, int device) {
    grom_chrom dc;
    grom_reads d, h = {0};
    if (grom_stage_view(st, ch, &dc, &d) != GROM_OK) return;
    h.n = d.n;
    h.n_cigar_ops = d.n_cigar_ops;
    h.n_bases = d.n_bases;
    h.n_aux = d.n_aux;
    h.n_drop = d.n_drop;
    const int64_t n = d.n, nd = d.n_drop;
#define DL(f, T, cnt)                                                                     \
    T *f##_h = (T *)malloc(sizeof(T) * (size_t)((cnt) > 0 ? (cnt) : 1));                   \
    if ((cnt) > 0 && d.f) grom_copy_d2h(f##_h, d.f, sizeof(T) * (size_t)(cnt), device);   \
    h.f = f##_h;
    DL(pos, int32_t, n) DL(flag, uint16_t, n) DL(mapq, uint8_t, n) DL(mtid, int32_t, n) DL(mpos, int32_t, n)
    DL(isize, int32_t, n) DL(l_qseq, int32_t, n) DL(cigar_off, uint32_t, n + 1) DL(base_off, int64_t, n)
    DL(name_id, uint32_t, n) DL(drop_pos, int32_t, nd) DL(drop_lq, int32_t, nd) DL(drop_before, int64_t, nd)
    /* absolute offsets: the whole CIGAR / base arrays */
    DL(cigar, uint32_t, d.n_cigar_ops) DL(qual, uint8_t, d.n_bases) DL(seq, uint8_t, d.n_bases / 2)
    DL(aux, grom_aux, d.n_aux)
#undef DL
    int32_t *ai = NULL;
    if (d.aux_idx) {
        ai = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n > 0 ? n : 1));
        if (n > 0) grom_copy_d2h(ai, d.aux_idx, sizeof(int32_t) * (size_t)n, device);
        h.aux_idx = ai;
    }
    printf("stage %s tid=%d reads=%lld n_skip=%d p_last=%d lseq_tail=%d digest=%016llx\n", ch->name, ch->tid,
           (long long)n, ch->n_skip, ch->p_last, ch->lseq_tail, (unsigned long long)pd_digest(&h));
    free((void *)h.pos); free((void *)h.flag); free((void *)h.mapq); free((void *)h.mtid); free((void *)h.mpos);
    free((void *)h.isize); free((void *)h.l_qseq); free((void *)h.cigar_off); free((void *)h.base_off);
    free((void *)h.name_id); free((void *)h.drop_pos); free((void *)h.drop_lq); free((void *)h.drop_before);
    free((void *)h.cigar); free((void *)h.qual); free((void *)h.seq); free((void *)h.aux); free(ai);
}

/* Scan one chromosome on context `slot`; its VCF rows go to j->text (malloc'd). */
/* the scan no longer reads the job's stage: the decoder may refill it while
 * the CNV path runs (grom_stage_on_consumed) */
static void job_stage_consumed(void *arg, grom_stage *st) {
    grom_job *j = (grom_job *)arg;
    j->stage_released = 1;
    pd_release_stage(j->pd, st);
}

static int scan_job(int slot, grom_job *j, cli_state *S) {
    const grom_params *P = &S->P;
    const cli_settings *E = &S->env;
    chrom_plan *cp = j->cp;
    j->text = j->ctx_text = NULL;
    j->text_len = j->ctx_len = 0;
    if (!chrom_wanted(S, cp->name)) return GROM_OK; /* serial path: another rank's chromosome */
    grom_chrom ch = {0};
    grom_reads rd = {0};
    int64_t n_reads;
    if (j->has_batch) {
        grom_batch *b = &j->batch;
        grom_batch_finish(b, P->one_base_rd_len / 4 + 1, P->overlap_mult, P->insert_max_size);
        ch.lseq_tail = b->lseq_tail;
        ch.n_skip = b->n_skip;
        ch.p_last = b->p_last;
        grom_batch_view(b, &rd);
        n_reads = b->n;
    } else {
        ch.lseq_tail = j->facts.lseq_tail;
        ch.n_skip = j->facts.n_skip;
        ch.p_last = j->facts.p_last;
        n_reads = j->facts.n_reads;
        if (E->plan_only) pd_mirror_view(j->pd, j->k, &rd); /* (host tests: the decoder's host mirror) */
    }
    if (E->plan_only) {
        printf("plan %s tid=%d reads=%lld n_skip=%d p_last=%d lseq_tail=%d digest=%016llx\n", cp->name, cp->tid,
               (long long)n_reads, ch.n_skip, ch.p_last, ch.lseq_tail, (unsigned long long)pd_digest(&rd));
        return GROM_OK;
    }
    ch.ref = cp->ref;
    ch.len = cp->len;
    ch.name = cp->name;
    ch.tid = cp->tid;
    ch.cnv = cp->tid >= 0; /* detect_del_dup runs for a matched target, GROM.c:16633 */
    ch.seed = E->has_seed ? E->seed : (uint32_t)time(NULL); /* srand(time()) per chromosome, GROM.c:1584 */
    if (!j->has_batch && E->stage_digest) stage_digest_line(j->stage, &ch, j->device);
    grom_out out = {0};
    grom_stats st = {0};
    /* the pileup's input sizes (the verbose line) before the stage is given back */
    int64_t n_cig = rd.n_cigar_ops, n_b = rd.n_bases;
    if (!j->has_batch) {
        grom_chrom dc;
        grom_reads dr;
        if (grom_stage_view(j->stage, &ch, &dc, &dr) == GROM_OK) {
            n_cig = dr.n_cigar_ops;
            n_b = dr.n_bases;
        }
        /* (GROM_DUMP reads the stage after the scan: it keeps it) */
        grom_stage_on_consumed(j->stage, j->pd && !E->dump ? job_stage_consumed : NULL, j);
    }
    if (j->pd) pd_trace(j->pd, PD_EV_SCAN, j->k, 0);
    int rc = j->has_batch ? grom_scan_chrom(slot, &ch, &rd, &out, &st)
                          : grom_scan_chrom_staged(slot, j->stage, &ch, &out, &st);
    if (j->pd) pd_trace(j->pd, PD_EV_SCAN, j->k, 1);
    if (rc != GROM_OK) {
        fprintf(stderr, "grom: scan of %s failed: %s\n", cp->name, grom_last_error());
        grom_out_free(&out);
        return rc;
    }
    j->text = out.vcf;
    j->text_len = out.vcf_len;
    j->ctx_text = out.ctx; /* raw CTX rows for the translocation post-pass */
    j->ctx_len = out.ctx_len;
    if (out.side_written && S->side_base) { /* -N: <results>.1000gen.<chr>, GROM.c:20246-20267 */
        char fn[4096];
        snprintf(fn, sizeof(fn), "%s.1000gen.%s", S->side_base, cp->name);
        FILE *f = fopen(fn, "w");
        if (!f) {
            printf("\nCould not open %s\n", fn);
            free(out.side);
            return GROM_E_ARG;
        }
        if (out.side_len) fwrite(out.side, 1, out.side_len, f);
        fclose(f);
    }
    free(out.side);
    if (E->dump) write_dumps(E->dump, slot, cp, &ch, &rd, j->has_batch ? NULL : j->stage, P);
    if (E->verbose) {
        /* the pileup kernel's launch and its inputs' sizes (bench.py's roofline) */
        printf("%s: %lld reads, %.3f ms on GPU (%.2f Mbases/s); pileup %.3f ms, cnv %.3f ms, cigar_ops %lld, "
               "bases %lld, len %ld\n", cp->name, (long long)n_reads, st.ms_total,
               st.ms_total > 0 ? cp->len / (st.ms_total * 1e3) : 0.0, st.ms_pileup, st.ms_cnv, (long long)n_cig,
               (long long)n_b, (long)cp->len);
    }
    return GROM_OK;
}

/* ---- multi-GPU: chromosomes shard across devices ----
 * The reference's -P forks one process per chromosome (GROM.c:328-624).  Here
 * -P n (or GROM_DEVICES) runs GROM_SCANS_PER_GPU worker threads per GPU, each
 * with its own library context.  Streamed input: every chromosome is staged
 * on the GPU chosen for it (longest-processing-time over the index's record
 * counts) and scanned by one of that GPU's workers.  Rows are written in
 * chromosome order, so the VCF is the same bytes as a one-GPU run. */

/* a finished chromosome: its VCF rows go out, its raw CTX rows are kept */
static void take_rows(cli_state *S, grom_job *j, FILE *vcf, textbuf *ctx_all) {
    if (j->text_len && S->env.vcf_segs) {
        const char *tab = memchr(j->text, '\t', j->text_len);
        char line[320];
        const int nl = tab ? (int)(tab - j->text) : 0;
        const int k = snprintf(line, sizeof(line), "%.*s\t%ld\t%zu\n", nl < 256 ? nl : 256, j->text, ftell(vcf),
                               (size_t)j->text_len);
        if (k > 0) textbuf_add(&S->vcf_segs, line, (size_t)k);
    }
    if (j->text_len) fwrite(j->text, 1, j->text_len, vcf);
    free(j->text);
    j->text = NULL;
    if (j->ctx_len) textbuf_add(ctx_all, j->ctx_text, j->ctx_len);
    free(j->ctx_text);
    j->ctx_text = NULL;
}

typedef struct grom_pool grom_pool;

typedef struct {
    grom_pool *pool;
    pthread_t thr;
    int slot;   /* the worker's own library context (grom_ctx_init) */
    int device; /* its GPU */
} grom_worker;

struct grom_pool {
    pthread_mutex_t mu;
    pthread_cond_t cv;
    grom_job *jobs; /* NULL: not started */
    int n_jobs, closing;
    cli_state *S;
    const int *pos; /* pos[k]: the job of the k-th chromosome in BAM order (NULL: job k) */
    grom_worker *workers;
    /* the rows' way out, on the thread that hands the chromosomes over */
    FILE *vcf;
    textbuf ctx_all;
    int next_write, status;
};

static void *grom_worker_main(void *arg) {
    grom_worker *w = (grom_worker *)arg;
    grom_pool *pl = w->pool;
    int cur = 0; /* jobs before `cur` are taken or belong to other GPUs */
    for (;;) {
        pthread_mutex_lock(&pl->mu);
        grom_job *j = NULL;
        for (;;) {
            while (cur < pl->n_jobs && pl->jobs[cur].ready &&
                   (pl->jobs[cur].taken || (pl->jobs[cur].device >= 0 && pl->jobs[cur].device != w->device)))
                cur++;
            if (cur < pl->n_jobs && pl->jobs[cur].ready) { j = &pl->jobs[cur]; break; }
            if (pl->closing) break;
            pthread_cond_wait(&pl->cv, &pl->mu);
        }
        if (!j) {
            pthread_mutex_unlock(&pl->mu);
            break;
        }
        j->taken = 1;
        pthread_mutex_unlock(&pl->mu);
        /* contexts are independent: workers sharing a GPU scan concurrently */
        int rc = scan_job(w->slot, j, pl->S);
        if (rc != GROM_OK) snprintf(j->err, sizeof(j->err), "%s: %s", j->cp->name, grom_last_error());
        free(j->cp->ref);
        j->cp->ref = NULL;
        plan_release_dref(pl->S, j->cp);
        if (j->has_batch) grom_batch_free(&j->batch);
        if (j->stage && j->pd && !j->stage_released) pd_release_stage(j->pd, j->stage);
        j->stage = NULL;
        pthread_mutex_lock(&pl->mu);
        j->rc = rc;
        j->done = 1;
        pthread_cond_broadcast(&pl->cv);
        pthread_mutex_unlock(&pl->mu);
    }
    return NULL;
}

/* Peak device memory of this process (GROM_VERBOSE): the kernel driver's
 * per-process VRAM count (/sys/class/kfd/kfd/proc/<pid>/vram_<gpu>), sampled
 * every 5 ms; without it, the device-wide use above the start's.  Printed as
 * the "footprint:" line, which bench.py reports. */
typedef struct {
    pthread_t thr;
    int started, stop, device, kfd;
    int64_t peak, base;
    double t_peak;
    pthread_mutex_t mu;
    pthread_cond_t cv;
} fp_sampler;

static int64_t fp_kfd_bytes(void) {
    char dir[96], path[384], buf[64];
    snprintf(dir, sizeof(dir), "/sys/class/kfd/kfd/proc/%d", (int)getpid());
    DIR *d = opendir(dir);
    if (!d) return -1;
    int64_t tot = 0;
    int any = 0;
    struct dirent *e;
    while ((e = readdir(d)) != NULL) {
        if (strncmp(e->d_name, "vram_", 5) != 0) continue;
        snprintf(path, sizeof(path), "%s/%s", dir, e->d_name);
        FILE *f = fopen(path, "r");
        if (!f) continue;
        if (fgets(buf, sizeof(buf), f)) { tot += atoll(buf); any = 1; }
        fclose(f);
    }
    closedir(d);
    return any ? tot : -1;
}

static void *fp_main(void *arg) {
    fp_sampler *F = (fp_sampler *)arg;
    F->kfd = fp_kfd_bytes() >= 0;
    if (!F->kfd) F->base = grom_device_mem_free(F->device);
    const double t0 = clock_gettime_s();
    pthread_mutex_lock(&F->mu);
    while (!F->stop) {
        pthread_mutex_unlock(&F->mu);
        int64_t v = F->kfd ? fp_kfd_bytes() : grom_device_mem_free(F->device);
        if (!F->kfd && v >= 0) v = F->base - v; /* base: free bytes at the start */
        pthread_mutex_lock(&F->mu);
        if (v > F->peak) { F->peak = v; F->t_peak = clock_gettime_s() - t0; }
        struct timespec ts;
        clock_gettime(CLOCK_REALTIME, &ts);
        ts.tv_nsec += 5000000;
        if (ts.tv_nsec >= 1000000000) { ts.tv_sec++; ts.tv_nsec -= 1000000000; }
        if (!F->stop) pthread_cond_timedwait(&F->cv, &F->mu, &ts);
    }
    pthread_mutex_unlock(&F->mu);
    return NULL;
}

static void fp_start(fp_sampler *F, int device) {
    memset(F, 0, sizeof(*F));
    F->device = device;
    pthread_mutex_init(&F->mu, NULL);
    pthread_cond_init(&F->cv, NULL);
    F->started = pthread_create(&F->thr, NULL, fp_main, F) == 0;
}

/* (since_start < 0: the sampler only ends, no line) */
static void fp_stop(fp_sampler *F, double since_start) {
    if (!F->started) return;
    pthread_mutex_lock(&F->mu);
    F->stop = 1;
    pthread_cond_broadcast(&F->cv);
    pthread_mutex_unlock(&F->mu);
    pthread_join(F->thr, NULL);
    F->started = 0;
    if (since_start < 0) return;
    int64_t pk[GROM_DEVCAT_N + 1], nw = 0, ns = 0;
    double sw = 0, ss = 0;
    grom_dev_peaks(pk, NULL);
    grom_dev_waits(&nw, &sw);
    grom_dev_slow(&ns, &ss);
    printf("footprint: peak %.2f GB of device memory (%s), at %.3f s of %.3f s; buffers: peak %.2f GB together, "
           "per kind scan %.2f, breakpoint %.2f, CNV %.2f, stages %.2f, decode %.2f, phase arenas %.2f GB; %lld "
           "allocations waited %.3f s for memory; %lld slow hipMalloc calls %.3f s\n", F->peak / 1e9,
           F->kfd ? "this process, kfd" : "device-wide use above the start's", F->t_peak, since_start,
           pk[GROM_DEVCAT_N] / 1e9, pk[GROM_DEVCAT_SCAN] / 1e9, pk[GROM_DEVCAT_SV] / 1e9, pk[GROM_DEVCAT_CNV] / 1e9,
           pk[GROM_DEVCAT_STAGE] / 1e9, pk[GROM_DEVCAT_DECODE] / 1e9, pk[GROM_DEVCAT_ARENA] / 1e9, (long long)nw, sw,
           (long long)ns, ss);
    pthread_mutex_destroy(&F->mu);
    pthread_cond_destroy(&F->cv);
    F->started = 0;
}

static void *hip_init_main(void *arg) {
    const cli_state *S = (const cli_state *)arg;
    (void)grom_device_count();
    if (!S->env.no_warm) dd_device_warm(S->device);
    /* the device decoder's first context, made while the host reads the
     * FASTA lengths and the BAI (GROM_NO_CTX_PREPARE=1: made by the worker).
     * One context is prepared: with several decode workers per GPU
     * (GROM_DD_WORKERS > 1) the first to start takes it, the others make
     * their own */
    if (S->env.device_decode != 0 && !S->env.no_ctx_prepare) dd_ctx_prepare(S->device);
    return NULL;
}

static void hip_start(cli_state *S) {
    S->hip_started = pthread_create(&S->hip_thr, NULL, hip_init_main, S) == 0;
}

static void hip_ready(cli_state *S) {
    if (S->hip_started) {
        pthread_join(S->hip_thr, NULL);
        S->hip_done = 1;
    }
    S->hip_started = 0;
}

/* the serial reader: after a fallback, or asked for (GROM_SERIAL_DECODE) */
static int reads_serially(const cli_state *S) { return S->force_serial || S->env.serial_decode; }

/* the host table and loader for -r.  `d`: the device loader gave up on the
 * file (NULL: it was never opened); `why`: the library's reason goes with a refusal */
static int fasta_host_fallback(cli_state *S, grom_fasta_dev **d, int why) {
    if (d) {
        fprintf(stderr, "grom: reading %s on the host\n", S->fasta_name);
        grom_fasta_dev_close(*d);
        grom_fasta_close(&S->fa);
    }
    if (grom_fasta_open_cached(&S->fa, S->fasta_name) == 0) return 0;
    printf("\nCould not open %s\n", S->fasta_name);
    if (why) printf("%s\n", grom_last_error());
    return -1;
}

/* The -r file opened.  Plain text: the host table and loader, as ever
 * (GROM_FASTA_DEVICE=1: the device loader).  BGZF: the device loader
 * (GROM_FASTA_DEVICE=0, the serial reader and plan-only runs: inflated on the
 * host).  A gzip file that is not BGZF, with GROM_FASTA_GZIP=1: BGZF's routes
 * (else refused).  <fasta>.info is read and written either way; for a
 * compressed file its file_pos are offsets in the inflated text.  The device
 * open waits for the HIP start-up thread. */
static int cli_fasta_open(cli_state *S) {
    const int kind = grom_fasta_file_kind(S->fasta_name), fd = S->env.fasta_device;
    const int gz = kind == 2 && grom_fasta_gzip_allowed(); /* a gzip file read as it is: BGZF's routes */
    const int want = ((kind == 1 || gz) && fd != 0) || (kind == 0 && fd == 1);
    if ((kind == 2 && !gz) || !want || reads_serially(S) || S->env.plan_only) return fasta_host_fallback(S, NULL, kind == 2);
    hip_start(S);
    memset(&S->fa, 0, sizeof(S->fa));
    grom_fasta_info_load(&S->fa, S->fasta_name);
    const long kept = S->fa.n > 0 ? 0 : S->fa.mappable;
    hip_ready(S);
    grom_fasta_dev *d = NULL;
    const int orc = grom_fasta_dev_open(S->fasta_name, S->device, &d);
    /* "host only": a gzip stream with a stretch too long for one lane */
    if (orc == GROM_FASTA_HOST_ONLY) return fasta_host_fallback(S, &d, 1);
    if (orc != 0) {
        printf("\nCould not open %s\n%s\n", S->fasta_name, grom_last_error());
        return -1;
    }
    int rc = 0;
    if (S->fa.n > 0) {
        int64_t *fp = malloc(sizeof(int64_t) * S->fa.n), *ln = malloc(sizeof(int64_t) * S->fa.n);
        for (int i = 0; i < S->fa.n; i++) { fp[i] = S->fa.file_pos[i]; ln[i] = S->fa.len[i]; }
        rc = grom_fasta_dev_set_index(d, S->fa.n, S->fa.mappable, (const char *)S->fa.names, S->fa.name_len, fp, ln);
        free(fp);
        free(ln);
    } else {
        int n = 0;
        int64_t mappable = 0;
        rc = grom_fasta_dev_index(d, &n, &mappable);
        if (rc == 0 && grom_fasta_reserve(&S->fa, n) != 0) rc = GROM_E_NOMEM;
        if (rc == 0) {
            for (int i = 0; i < n; i++) {
                int64_t fp = 0, ln = 0;
                grom_fasta_dev_entry(d, i, S->fa.names[i], &S->fa.name_len[i], &fp, &ln, NULL);
                S->fa.file_pos[i] = (long)fp;
                S->fa.len[i] = (long)ln;
            }
            S->fa.n = n;
            S->fa.mappable = (long)mappable + kept;
            grom_fasta_info_save(&S->fa, S->fasta_name);
        }
    }
    if (rc != 0) { /* "host only", or the device pass failed */
        if (rc != GROM_FASTA_HOST_ONLY) fprintf(stderr, "grom: device FASTA loader: %s\n", grom_last_error());
        return fasta_host_fallback(S, &d, 0);
    }
    S->fdev = d;
    return 0;
}

#define CLI_FALLBACK 99 /* the streamed path could not be used: read serially */

static void *tables_main(void *arg) {
    cli_state *S = (cli_state *)arg;
    grom_build_tables(S->P.min_mapq, S->hez, S->mq); /* read_binom_tables, GROM.c:22234 */
    return NULL;
}

static void tables_join(cli_state *S) {
    if (S->tables_started) pthread_join(S->tables_thr, NULL);
    S->tables_started = 0;
}

/* The run's device plan, derived here alone from the settings, -P and the
 * free-memory query: the GPUs (GROM_DEVICES over -P n, at most those present
 * from `device` on and at most 64), the scan contexts per GPU
 * (GROM_SCANS_PER_GPU, default 2, so two chromosomes are in flight on every
 * GPU), the worker -> GPU list and the streamed run's stages per GPU
 * (GROM_STAGES).  GROM_WORKER_DEVICES=0,0,0 (test hook) runs three workers on
 * device 0; a streamed run then has four stages, on the first listed device.
 * `fit_hbm`: the contexts are about to be made (setup_workers), so their count
 * is cut to what the free HBM holds now, after the stages took their share;
 * the streamed run plans its stages and decoder before that, without it. */
static int plan_devices(cli_state *S, int fit_hbm) {
    const cli_settings *E = &S->env;
    if (E->devices) S->n_dev = E->devices;
    if (S->n_dev < 1) S->n_dev = 1;
    if (!E->plan_only && S->n_dev > 1) {
        int avail = grom_device_count();
        if (avail < 1) { fprintf(stderr, "grom: no GPU\n"); return -1; }
        if (S->n_dev > avail - S->device) S->n_dev = avail - S->device;
        if (S->n_dev < 1) S->n_dev = 1;
    }
    if (S->n_dev > CLI_MAX_WORKERS) S->n_dev = CLI_MAX_WORKERS;
    int per_gpu = E->scans_per_gpu;
    if (per_gpu * S->n_dev > CLI_MAX_WORKERS) per_gpu = CLI_MAX_WORKERS / S->n_dev;
    /* a second context per GPU doubles the scan's device buffers: keep it
     * only when the free HBM holds per_gpu scans of the longest chromosome
     * (about 64 B per base at 30x) */
    if (fit_hbm && per_gpu > 1 && !E->plan_only) {
        long longest = 0;
        for (int i = 0; i < S->fa.n; i++)
            if (S->fa.len[i] > longest) longest = S->fa.len[i];
        const double need = 64.0 * (double)longest;
        for (int d = 0; d < S->n_dev; d++) {
            int64_t fr = grom_device_mem_free(S->device + d);
            if (fr >= 0 && (double)fr < need * per_gpu) {
                int fit = (int)((double)fr / need);
                per_gpu = fit < 1 ? 1 : (fit < per_gpu ? fit : per_gpu);
            }
        }
    }
    S->n_work = S->n_dev * per_gpu;
    for (int d = 0; d < CLI_MAX_WORKERS; d++) S->wdev[d] = S->device + d % S->n_dev;
    if (E->n_worker_devices >= 0) {
        S->n_work = E->n_worker_devices;
        memcpy(S->wdev, E->worker_devices, sizeof(int) * (size_t)S->n_work);
        if (S->n_work < 1) { S->wdev[0] = S->device; S->n_work = 1; }
    }
    return 0;
}

/* the scan workers' library contexts (they get their insert parameters later) */
static int setup_workers(cli_state *S) {
    if (plan_devices(S, 1)) return -1;
    tables_join(S);
    hip_ready(S);
    int rc = GROM_OK;
    for (int d = 0; d < S->n_work && !S->env.plan_only && rc == GROM_OK; d++) {
        rc = grom_ctx_init(d, S->wdev[d], &S->P, S->hez, S->mq);
        if (rc == GROM_OK) S->n_init = d + 1;
    }
    if (rc != GROM_OK) { fprintf(stderr, "grom: %s\n", grom_last_error()); return -1; }
    return 0;
}

/* The order chromosomes are best taken in: idx[0..n) sorted longest first,
 * chromosomes of one length in their given order (a stable insertion sort) */
static void longest_first(int *idx, int n, chrom_plan *const *p) {
    for (int a = 1; a < n; a++)
        for (int b = a; b > 0 && p[idx[b]]->len > p[idx[b - 1]]->len; b--) {
            const int t = idx[b];
            idx[b] = idx[b - 1];
            idx[b - 1] = t;
        }
}

/* the insert lines and <bam>.mean (save_insert_mean, GROM.c:994-1008), or
 * `given`: the statistics came from that file; a serial rerun prints nothing
 * twice (insert_printed) */
static void print_insert(cli_state *S, int given, int imean, int lseq, int imin, int imax, long mapped) {
    const int quiet = *S->insert_printed && !given;
    *S->insert_printed = 1;
    char mean_name[4096];
    snprintf(mean_name, sizeof(mean_name), "%s.mean", S->bam_name);
    if (given) printf("Loading insert_mean et al from %s\n", mean_name);
    else if (!quiet) printf("insert_min_size, insert_max_size %d %d\n", imin, imax);
    FILE *mf = given ? NULL : fopen(mean_name, "w");
    if (mf) {
        if (!quiet) printf("Saving insert_mean et al to %s\n", mean_name);
        fprintf(mf, "%d %d %d %d %ld\n", imean, lseq, imin, imax, mapped);
        fclose(mf);
    }
    grom_params_set_insert(&S->P, imean, imin, imax, lseq);
    if (quiet) return;
    printf("insert mean, insert minimum, insert maximum: %d %d %d\n", S->P.insert_mean, imin, imax);
    printf("median read length: %d\n", lseq);
}

/* find_disc_svs' length test (GROM.c:20826-21050), needs the insert size */
static int passes_length(const cli_state *S, const chrom_plan *c) {
    const int32_t s0 = S->P.one_base_rd_len / 4 + 1;
    if (c->len > S->max_chr_len)
        printf("ERROR: Reference chromosome length exceeds maximum allowed chromosome size (%ld)\n", S->max_chr_len);
    return c->len > s0 + (long)S->P.overlap_mult * S->P.insert_max_size && c->len > 0 && c->len <= S->max_chr_len;
}

/* GROM_VCF_BGZF: a FILE whose bytes go to a BGZF writer on the run's first
 * device (grom_bgzf_writer_*); fclose closes the writer, which
 * frees its device memory, and keeps its counters in out[10] */
typedef struct {
    grom_bgzf_writer *w;
    grom_vcf_writer *vw; /* GROM_VCF_TABIX: the sorting, indexing writer instead */
    cli_state *S;
    int64_t *out;
} gz_cookie;

static ssize_t gz_cookie_write(void *c, const char *buf, size_t n) {
    gz_cookie *g = c;
    const int rc = g->vw ? grom_vcf_writer_write(g->vw, buf, (int64_t)n) : grom_bgzf_writer_write(g->w, buf, (int64_t)n);
    if (rc != 0) { g->S->gz_failed = 1; return 0; }
    return (ssize_t)n;
}

static int gz_cookie_close(void *c) {
    gz_cookie *g = c;
    const int rc = g->vw ? grom_vcf_writer_close(g->vw, g->out) : grom_bgzf_writer_close(g->w, g->out);
    if (rc != 0) {
        g->S->gz_failed = 1;
        printf("Error writing %s output: %s\n", g->vw ? "sorted, indexed VCF" : "BGZF", grom_last_error());
    }
    free(g);
    return rc ? -1 : 0;
}

static FILE *gz_fopen(cli_state *S, const char *name, int with_gzi, int64_t *out) {
    char gzi[4200];
    snprintf(gzi, sizeof(gzi), "%s.gzi", name);
    hip_ready(S);
    gz_cookie *g = calloc(1, sizeof(*g));
    g->S = S;
    g->out = out;
    if (S->env.vcf_tabix) g->vw = grom_vcf_writer_open(name, S->device);
    else g->w = grom_bgzf_writer_open(name, S->device, with_gzi ? gzi : NULL);
    if (!g->w && !g->vw) { free(g); return NULL; }
    const cookie_io_functions_t io = {NULL, gz_cookie_write, NULL, gz_cookie_close};
    FILE *f = fopencookie(g, "w", io);
    if (!f) {
        if (g->vw) grom_vcf_writer_close(g->vw, NULL);
        else grom_bgzf_writer_close(g->w, NULL);
        free(g);
        return NULL;
    }
    setvbuf(f, NULL, _IOFBF, 1 << 20);
    return f;
}

/* the rows' file, under its header */
static FILE *open_rows(cli_state *S) {
    FILE *vcf = S->env.vcf_bgzf ? gz_fopen(S, S->gz_name, 1, S->gz_rows) : fopen(S->out_name, "w");
    if (!vcf) { printf("Error opening file %s\n", S->env.vcf_bgzf ? S->gz_name : S->out_name); return NULL; }
    if (S->one_chrom < 0) { /* (-c: rows only, the parent wrote the header) */
        if (S->P.vcf == 1) header(vcf, S->fasta_name, 0, S->env.filedate);
        else tab_header(vcf, &S->P);
    }
    return vcf;
}

static void write_file(const char *name, const textbuf *t) {
    FILE *f = fopen(name, "w");
    if (!f) return;
    if (t->len) fwrite(t->p, 1, t->len, f);
    fclose(f);
}

static void finish_outputs(cli_state *S, textbuf *ctx_all) {
    if (S->env.vcf_segs) write_file(S->env.vcf_segs, &S->vcf_segs);
    /* -c: the raw CTX rows; the parent pairs them (GROM.c:22400) */
    if (S->one_chrom >= 0) { write_file(S->ctx_name, ctx_all); return; }
    if (S->env.ctx_raw) write_file(S->env.ctx_raw, ctx_all); /* for a merge of several ranks' runs */
    /* CTX post-pass (GROM.c:22400-22770): pair the translocation rows of all
     * chromosomes with their mates and write them under the header */
    FILE *ctx = S->env.vcf_bgzf ? gz_fopen(S, S->ctx_gz_name, 0, S->gz_ctx) : fopen(S->ctx_name, "w");
    if (ctx) {
        if (S->P.vcf == 1) header(ctx, S->fasta_name, 1, S->env.filedate);
        else /* the trimmed file's column header, GROM.c:22652-22700 */
            fputs("SV\tChromosome\tStart\tID\tMate ID\tBinom Prob (Start)\tCTX evidence\tRead Depth (High MapQ)\t"
                  "Concordant Pairs\tOther (Number of Non-Empty)\tMate Chr\tMate Pos\tRead Start\tRead End\t"
                  "Hez binom prob\n", ctx);
        ctx_postpass(ctx_all->p, ctx_all->len, &S->hdr, S->P.insert_max_size, S->P.lseq, S->P.vcf == 1, ctx);
        fclose(ctx);
    }
    if (S->env.vcf_tabix && !S->gz_failed)
        printf("Sorted, indexed output (device %d): %s with %s.tbi and %s.gzi, %lld rows on %lld contigs, %lld inversions, "
               "%lld radix passes, %lld bins; %s with its .tbi and .gzi, %lld rows on %lld contigs; %.3f s on the device\n",
               S->device, S->gz_name, S->gz_name, S->gz_name, (long long)S->gz_rows[0], (long long)S->gz_rows[2],
               (long long)S->gz_rows[3], (long long)S->gz_rows[4], (long long)S->gz_rows[5], S->ctx_gz_name,
               (long long)S->gz_ctx[0], (long long)S->gz_ctx[2],
               (double)(S->gz_rows[8] + S->gz_rows[9] + S->gz_rows[10] + S->gz_ctx[8] + S->gz_ctx[9] + S->gz_ctx[10]) / 1e6);
    else if (S->env.vcf_bgzf && !S->gz_failed)
        printf("BGZF output (device %d): %s with %s.gzi, %lld blocks, %lld -> %lld bytes; %s, %lld blocks, %lld -> %lld bytes; "
               "%.3f s on the device\n", S->device, S->gz_name, S->gz_name, (long long)S->gz_rows[0], (long long)S->gz_rows[5],
               (long long)S->gz_rows[6], S->ctx_gz_name, (long long)S->gz_ctx[0], (long long)S->gz_ctx[5],
               (long long)S->gz_ctx[6], (double)(S->gz_rows[8] + S->gz_ctx[8]) / 1e6);
}

/* rows of finished jobs, in chromosome order (caller holds pool.mu) */
static void drain_rows(grom_pool *pool, int upto) {
    while (pool->next_write < upto && pool->jobs[pool->pos ? pool->pos[pool->next_write] : pool->next_write].done) {
        grom_job *j = &pool->jobs[pool->pos ? pool->pos[pool->next_write] : pool->next_write];
        pool->next_write++;
        pthread_mutex_unlock(&pool->mu);
        if (j->rc != GROM_OK) pool->status = 1;
        take_rows(pool->S, j, pool->vcf, &pool->ctx_all);
        pthread_mutex_lock(&pool->mu);
    }
}

static void pool_start(grom_pool *pool, cli_state *S, int n_jobs) {
    pthread_mutex_init(&pool->mu, NULL);
    pthread_cond_init(&pool->cv, NULL);
    pool->jobs = calloc(n_jobs > 0 ? n_jobs : 1, sizeof(grom_job));
    pool->n_jobs = n_jobs;
    pool->S = S;
    pool->workers = calloc(S->n_work, sizeof(grom_worker));
    for (int d = 0; d < S->n_work; d++) {
        pool->workers[d] = (grom_worker){.pool = pool, .slot = d, .device = S->wdev[d]};
        pthread_create(&pool->workers[d].thr, NULL, grom_worker_main, &pool->workers[d]);
    }
}

/* close the pool: wait for every job, write the remaining rows */
static void pool_finish(grom_pool *pool) {
    pthread_mutex_lock(&pool->mu);
    pool->closing = 1;
    pthread_cond_broadcast(&pool->cv);
    for (;;) {
        drain_rows(pool, pool->n_jobs);
        int busy = 0;
        for (int j = 0; j < pool->n_jobs; j++)
            if (pool->jobs[j].ready && !pool->jobs[j].done) busy = 1;
        if (!busy) break;
        pthread_cond_wait(&pool->cv, &pool->mu);
    }
    pthread_mutex_unlock(&pool->mu);
    for (int d = 0; d < pool->S->n_work; d++) pthread_join(pool->workers[d].thr, NULL);
    for (int j = 0; j < pool->n_jobs; j++)
        if (pool->jobs[j].ready && pool->jobs[j].rc != GROM_OK) { grom_set_last_error(pool->jobs[j].err); pool->status = 1; break; }
    free(pool->workers);
    free(pool->jobs);
    pthread_mutex_destroy(&pool->mu);
    pthread_cond_destroy(&pool->cv);
}

/* ---------------- serial input: one pass over the record stream ---------------- */
typedef struct {
    cli_state *S;
    bgzf_reader br;
    int br_open;
    chrom_plan **plan; /* the final plan: candidates that pass the length test */
    int32_t *order;    /* their BAM targets */
    int n_plan, cur;   /* `cur`: the chromosome whose records are being read */
    grom_batch batch;
    int batch_ended;   /* the record after the chromosome's last one was seen */
    bam_rec rec;
    grom_pool pool;
} serial_run;

/* the BAM opened at its first record; `threads`: its blocks inflate on so many threads */
static int serial_open(serial_run *R, const int *threads) {
    if (bgzf_open_read(&R->br, R->S->bam_name) != 0) return 1;
    R->br_open = 1;
    if (threads && bgzf_set_threads(&R->br, *threads) != 0) return 1;
    bam_hdr h2;
    if (bam_read_header(&R->br, &h2) != 0) return 1;
    bam_free_header(&h2);
    return 0;
}

static void serial_batch_init(serial_run *R) {
    if (R->cur >= R->n_plan) return;
    grom_batch_init(&R->batch, R->order[R->cur], R->S->P.read_name_len);
    grom_batch_set_sv(&R->batch, R->plan[R->cur]->target, R->S->P.splitread);
    R->batch_ended = 0;
}

/* hand chromosome `cur` (its batch complete) to the workers; at most one
 * decoded chromosome waits beyond those being scanned */
static void serial_submit(serial_run *R) {
    grom_pool *pool = &R->pool;
    chrom_plan *c = R->plan[R->cur];
    c->ref = malloc(c->len + 1);
    grom_fasta_load(&R->S->fa, c->fasta_idx, c->ref, c->len);
    pthread_mutex_lock(&pool->mu);
    grom_job *j = &pool->jobs[R->cur];
    j->cp = c;
    j->batch = R->batch;
    j->has_batch = 1;
    j->device = -1;
    j->ready = 1;
    pthread_cond_broadcast(&pool->cv);
    for (;;) {
        drain_rows(pool, R->cur + 1);
        if (R->cur + 1 - pool->next_write < R->S->n_work + 1) break;
        pthread_cond_wait(&pool->cv, &pool->mu);
    }
    pthread_mutex_unlock(&pool->mu);
    R->cur++;
    serial_batch_init(R);
}

/* the insert-size pre-pass on the first records (GROM.c:22255), the scan
 * contexts, and the final plan */
static int serial_prepare(serial_run *R) {
    cli_state *S = R->S;
    if (serial_open(R, NULL)) return 1;
    int lseq = 0, imin = 0, imax = 0;
    long mapped = 0;
    int imean = grom_insert_stats(&R->br, grom_prob2(S->num_sd), &lseq, &imin, &imax, &mapped, S->P.min_mapq);
    bgzf_close_read(&R->br);
    R->br_open = 0;
    if (imean < 0) { printf("ERROR: no reads to estimate the insert size from\n"); return 1; }
    print_insert(S, 0, imean, lseq, imin, imax, mapped);
    if (setup_workers(S)) return 1;
    R->plan = calloc(S->n_cand > 0 ? S->n_cand : 1, sizeof(chrom_plan *));
    R->order = calloc(S->n_cand > 0 ? S->n_cand : 1, sizeof(int32_t));
    for (int c = 0; c < S->n_cand; c++)
        if (passes_length(S, &S->plan[c])) {
            R->order[R->n_plan] = S->plan[c].tid;
            R->plan[R->n_plan++] = &S->plan[c];
        }
    return 0;
}

/* One serial pass over the records, split per chromosome (stream.h); finished
 * chromosomes go to the GPU workers, rows are written in order.  BGZF blocks
 * inflate on GROM_DECODE_THREADS threads (default 4) while this thread parses
 * records in order (htslib's bgzf_mt) */
static void serial_read(serial_run *R) {
    const cli_state *S = R->S;
    const int32_t s0 = S->P.one_base_rd_len / 4 + 1;
    bam_rec *rec = &R->rec;
    grom_planner pl;
    grom_planner_init(&pl, R->order, R->n_plan);
    serial_batch_init(R);
    while (S->fetch && R->cur < R->n_plan && bam_read_rec(&R->br, rec) > 0) {
        /* -P: chromosome `cur` is given its own target's placed records
         * (bam_fetch over [0, MAX_REGION), GROM.c:320) and its stream ends at
         * its last one; a record of a later plan chromosome completes every
         * chromosome before it.  The file is coordinate-sorted (bam_fetch's
         * precondition): a record of an earlier target cannot follow. */
        if (rec->pos < 0 || rec->pos >= 300000000) continue;
        int k = -1;
        for (int j = R->cur; j < R->n_plan && k < 0; j++)
            if (R->order[j] == rec->tid) k = j;
        if (k < 0) {
            for (int j = 0; j < R->cur; j++)
                if (R->order[j] == rec->tid) {
                    fprintf(stderr, "grom: -P needs a coordinate-sorted BAM (target %d after a later one)\n", rec->tid);
                    R->pool.status = 1;
                }
            if (R->pool.status) break;
            continue;
        }
        while (R->cur < k) serial_submit(R);
        grom_batch_add(&R->batch, rec, s0);
    }
    while (!S->fetch && R->cur < R->n_plan && bam_read_rec(&R->br, rec) > 0) {
        /* cdp_lseq after the chromosome: the l_qseq of the record that ended
         * it (the R-side edge tests of its last bases read it, GROM.c:12047) */
        if (!R->batch_ended && R->batch.n_seen > 0 && rec->tid != R->order[R->cur]) {
            grom_batch_end_record(&R->batch, rec);
            R->batch_ended = 1;
        }
        int k = grom_planner_feed(&pl, rec->tid);
        while (R->cur < R->n_plan && pl.k > R->cur) serial_submit(R); /* chromosome `cur` is complete */
        if (k >= 0 && k == R->cur) grom_batch_add(&R->batch, rec, s0);
    }
    /* end of file: the chromosome being read and every later one */
    while (R->cur < R->n_plan) serial_submit(R);
}

static int run_serial(cli_state *S) {
    serial_run R = {.S = S};
    const int n_dec = S->env.has_decode_threads ? S->env.decode_threads : 4;
    int status = 1;
    if (!serial_prepare(&R) && (R.pool.vcf = open_rows(S)) != NULL && !serial_open(&R, &n_dec)) {
        pool_start(&R.pool, S, R.n_plan);
        serial_read(&R);
        pool_finish(&R.pool);
        status = R.pool.status;
    }
    bam_free_rec(&R.rec);
    if (R.br_open) bgzf_close_read(&R.br);
    if (R.pool.vcf) fclose(R.pool.vcf);
    if (R.pool.S) finish_outputs(S, &R.pool.ctx_all); /* (only a run whose pool started writes them) */
    free(R.pool.ctx_all.p);
    free(R.plan);
    free(R.order);
    return status;
}

/* ---------------- streamed input: parallel decode -> pinned pieces -> HBM ---------------- */
typedef struct {
    cli_state *S;
    chrom_plan **plan;
    int n_plan;
    pthread_mutex_t mu;
    pthread_cond_t cv;
    int loaded, consumed, stop; /* refs loaded (a prefix of the plan) ahead of the consumer, at most `ahead` */
    int ahead;
    int next;         /* the next chromosome a loader thread takes */
    char *done;       /* per chromosome: its reference is loaded (NULL: the feed was never set up) */
    pthread_t thr[8]; /* GROM_FASTA_THREADS' upper bound */
    int n_thr;
} fasta_feed;

/* A chromosome's reference buffer: 2 MB aligned and advised for huge pages,
 * so the first touch of a 250 MB chromosome is ~125 faults instead of ~61 k
 * (half of a single thread's load time went to page faults) */
static char *ref_alloc(long len) {
    const size_t huge = (size_t)2 << 20, n = ((size_t)len + 1 + huge - 1) / huge * huge;
    void *p = NULL;
    if (posix_memalign(&p, huge, n) != 0) return NULL;
#ifdef MADV_HUGEPAGE
    (void)madvise(p, n, MADV_HUGEPAGE);
#endif
    return (char *)p;
}

/* the host loader on a run that reads the FASTA on the device ("host only", a
 * failed device load): the stream is opened when first needed (a BGZF file is
 * inflated on the host) and read by one thread at a time */
static long cli_fasta_host_load(cli_state *S, int fi, char *buf, long cap) {
    static pthread_mutex_t fmu = PTHREAD_MUTEX_INITIALIZER;
    long r = -1;
    pthread_mutex_lock(&fmu);
    if (grom_fasta_attach(&S->fa, S->fasta_name) == 0) r = grom_fasta_load(&S->fa, fi, buf, cap);
    pthread_mutex_unlock(&fmu);
    return r;
}

/* find_disc_svs loads each chromosome in order (GROM.c:21009-21045); here a
 * few threads do it ahead of the scans (one thread at ~0.9 GB/s of FASTA was
 * slower than the GPU decode: the whole run waited on it), each taking the
 * next chromosome of the plan; `loaded` counts the plan's loaded prefix */
static void *fasta_main(void *arg) {
    fasta_feed *F = (fasta_feed *)arg;
    for (;;) {
        pthread_mutex_lock(&F->mu);
        const int k = F->next;
        if (k < F->n_plan) F->next++;
        while (!F->stop && k < F->n_plan && k >= F->consumed + F->ahead) pthread_cond_wait(&F->cv, &F->mu);
        const int stop = F->stop || k >= F->n_plan;
        pthread_mutex_unlock(&F->mu);
        if (stop) break;
        chrom_plan *c = F->plan[k];
        c->ref = ref_alloc(c->len);
        if (c->ref && F->S->fdev) {
            /* the device loader: the bytes stay in HBM for the stage and come back for the host's SV rows */
            pthread_mutex_lock(&F->S->fdev_mu);
            const int64_t r = grom_fasta_dev_load(F->S->fdev, c->fasta_idx, c->ref, c->len, &c->d_ref);
            pthread_mutex_unlock(&F->S->fdev_mu);
            if (r != c->len) {
                if (r != GROM_FASTA_HOST_ONLY) fprintf(stderr, "grom: device FASTA loader: %s; reading %s on the host\n", grom_last_error(), c->name);
                plan_release_dref(F->S, c);
                cli_fasta_host_load(F->S, c->fasta_idx, c->ref, c->len);
            }
        } else if (c->ref && grom_fasta_load_at(&F->S->fa, c->fasta_idx, c->ref, c->len) < 0) {
            /* (the shared-stream loader: one thread at a time) */
            static pthread_mutex_t fmu = PTHREAD_MUTEX_INITIALIZER;
            pthread_mutex_lock(&fmu);
            grom_fasta_load(&F->S->fa, c->fasta_idx, c->ref, c->len);
            pthread_mutex_unlock(&fmu);
        }
        pthread_mutex_lock(&F->mu);
        F->done[k] = 1;
        while (F->loaded < F->n_plan && F->done[F->loaded]) F->loaded++;
        pthread_cond_broadcast(&F->cv);
        pthread_mutex_unlock(&F->mu);
    }
    return NULL;
}

/* the CPUs this process may use: the cgroup's CPU quota when it has one
 * (cpu.max "quota period"; a container's share of a large host), else the
 * online CPUs -- more decoder threads than that only contend */
static int host_cpus(void) {
    long ncpu = sysconf(_SC_NPROCESSORS_ONLN);
    FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r");
    if (f) {
        char q[64] = "";
        long period = 0;
        if (fscanf(f, "%63s %ld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
            const long c = (atol(q) + period - 1) / period;
            if (c >= 1 && c < ncpu) ncpu = c;
        }
        fclose(f);
    }
    return ncpu < 1 ? 1 : (int)ncpu;
}

static void *stage_free_main(void *arg) {
    grom_stage_free((grom_stage *)arg);
    return NULL;
}

/* a streamed run: what its phases share, and what streamed_close releases */
typedef struct {
    cli_state *S;
    pd_session *pd;
    int *dev_of; /* candidate -> the GPU its stage and scan are on */
    grom_stage *stages[256];
    int n_stages;
    /* insert statistics read from <bam>.mean (`given`), else measured */
    int given, imean, lseq, imin, imax;
    long mapped;
    int status, fallback; /* the run failed; the serial reader has to take over */
    /* the final plan: wanted candidates that pass the length test, in BAM
     * order; pidx[k]: the k-th one's candidate */
    int *keep, *pidx, n_plan;
    chrom_plan **plan;
    /* the queue: the order chromosomes are taken in; qpos[k]: where the k-th of the plan stands in it */
    int *qord, *qpos;
    chrom_plan **qplan;
    fasta_feed F;
    grom_pool pool;
    double t_start, t_started, t_stats, t_ctx, t_loop;
} streamed_run;

/* longest processing time first over the chromosome lengths: every candidate's GPU */
static void assign_devices(const cli_state *S, int *dev_of) {
    const int n = S->n_cand;
    double load[CLI_MAX_WORKERS] = {0};
    int *idx = malloc(sizeof(int) * (n > 0 ? n : 1));
    chrom_plan **all = calloc(n > 0 ? n : 1, sizeof(chrom_plan *));
    for (int c = 0; c < n; c++) { idx[c] = c; all[c] = &S->plan[c]; }
    longest_first(idx, n, all);
    for (int a = 0; a < n; a++) {
        int best = 0;
        for (int d = 1; d < S->n_dev; d++)
            if (load[d] < load[best]) best = d;
        dev_of[idx[a]] = S->device + best;
        load[best] += (double)all[idx[a]]->len;
    }
    /* (GROM_WORKER_DEVICES, test hook: every chromosome on the stages' one device) */
    for (int c = 0; c < n && S->env.n_worker_devices >= 0; c++) dev_of[c] = S->wdev[0];
    free(idx);
    free(all);
}

/* phase 1: the decoder opened over the preliminary plan (every candidate: the
 * length test needs the insert size, which the same decode measures), the
 * stages made and the decode started */
static int streamed_open(streamed_run *R) {
    cli_state *S = R->S;
    const cli_settings *E = &S->env;
    const int n1 = S->n_cand > 0 ? S->n_cand : 1;
    pd_chrom_in *cin = calloc(n1, sizeof(pd_chrom_in));
    for (int c = 0; c < S->n_cand; c++) {
        cin[c].tid = S->plan[c].tid;
        cin[c].target_name = S->plan[c].target;
        cin[c].len = S->plan[c].len;
    }
    /* the host decoder's threads (GROM_DEVICE_DECODE=0 and plan-only runs):
     * the CPU share, at most 32 (its piece window grows with the count) */
    int n_thr = E->has_decode_threads ? E->decode_threads : (host_cpus() < 32 ? host_cpus() : 32);
    if (n_thr < 1) n_thr = 1;
    char why[256] = "";
    R->pd = pd_open(S->bam_name, &S->hdr, cin, S->n_cand, S->P.splitread, S->P.read_name_len, n_thr, why,
                    (int)sizeof(why));
    free(cin);
    if (!R->pd) {
        if (E->verbose) printf("streamed decode not used: %s\n", why);
        return CLI_FALLBACK;
    }
    /* GPUs: contexts need the insert statistics, stages do not */
    hip_ready(S);
    if (plan_devices(S, 0)) return 1;
    R->dev_of = calloc(5 * (size_t)n1, sizeof(int)); /* with keep, pidx, qord and qpos behind it */
    R->plan = calloc(2 * (size_t)n1, sizeof(chrom_plan *)); /* with qplan */
    assign_devices(S, R->dev_of);
    /* one stage per scan: a scan gives its stage back before its CNV path
     * (grom_stage_on_consumed), so the next chromosome decodes into it while
     * the CNV path runs.  A third stage (GROM_STAGES=3, the round-4/5
     * default) let the decode run one chromosome further ahead for 15.5 GB
     * more at 30x, and the whole run was no faster (profiles/r05r: 4.03-4.04 s
     * against 4.00-4.12 s) */
    const int hook = E->n_worker_devices >= 0; /* GROM_WORKER_DEVICES: four stages, on the first worker's device */
    const int dev0 = hook ? S->wdev[0] : S->device, gpus = hook ? 1 : S->n_dev, per_gpu = hook ? 4 : E->stages;
    for (int d = 0; d < gpus && !E->plan_only; d++)
        for (int k = 0; k < per_gpu && R->n_stages < 256; k++) {
            grom_stage *st = grom_stage_new(dev0 + d);
            if (!st) break;
            R->stages[R->n_stages++] = st;
            pd_add_stage(R->pd, st, dev0 + d);
        }
    /* a share of a multi-process run (GROM_CHROMS, bench.py --gpus N) reads
     * the insert statistics from <bam>.mean as the reference's -c children do
     * (load_insert_mean, GROM.c:1011-1026, 22253-22257) */
    if ((E->chroms || S->one_chrom >= 0) && !E->plan_only) {
        char mean_name[4096];
        snprintf(mean_name, sizeof(mean_name), "%s.mean", S->bam_name);
        FILE *mf = fopen(mean_name, "r");
        if (mf) {
            R->given = fscanf(mf, "%d %d %d %d %ld", &R->imean, &R->lseq, &R->imin, &R->imax, &R->mapped) == 5 &&
                       R->imean > 0;
            fclose(mf);
        }
        if (R->given) pd_stats_given(R->pd);
    }
    if (S->fetch) pd_set_fetch_mode(R->pd, 1);
    if (E->chroms) {
        int *want = calloc(n1, sizeof(int));
        for (int c = 0; c < S->n_cand; c++) want[c] = chrom_wanted(S, S->plan[c].name);
        pd_set_wanted(R->pd, want);
        free(want);
    }
    /* BAM decode on the GPUs (ddecode.hip) by default; the host decoder
     * threads with GROM_DEVICE_DECODE=0 (plan-only runs always use them) */
    pd_set_device_mode(R->pd, !E->plan_only && E->device_decode != 0);
    if (pd_start(R->pd, S->P.min_mapq, S->n_dev, R->dev_of, E->plan_only)) {
        fprintf(stderr, "grom: %s\n", pd_error(R->pd));
        return 1;
    }
    R->t_started = clock_gettime_s();
    return 0;
}

/* phase 2: the insert statistics, given or measured from the head of the BAM,
 * with their printed lines (and, measured, <bam>.mean) */
static int streamed_insert_stats(streamed_run *R) {
    cli_state *S = R->S;
    if (!R->given)
        R->imean = pd_insert_stats(R->pd, grom_prob2(S->num_sd), S->P.min_mapq, &R->lseq, &R->imin, &R->imax, &R->mapped);
    if (R->imean < 0) {
        if (R->imean != -2) printf("ERROR: no reads to estimate the insert size from\n");
        else if (S->env.verbose) printf("streamed decode stopped: %s\n", pd_error(R->pd));
        return R->imean == -2 ? CLI_FALLBACK : 1;
    }
    print_insert(S, R->given, R->imean, R->lseq, R->imin, R->imax, R->mapped);
    R->t_stats = clock_gettime_s();
    return 0;
}

/* phase 3: the final plan, told to the decoder, and the queue order: the
 * device decoder's (longest first), else BAM order; rows are written in BAM
 * order either way */
static int streamed_plan(streamed_run *R) {
    cli_state *S = R->S;
    const int n1 = S->n_cand > 0 ? S->n_cand : 1;
    R->keep = R->dev_of + n1;
    R->pidx = R->keep + n1;
    for (int c = 0; c < S->n_cand; c++)
        if ((R->keep[c] = passes_length(S, &S->plan[c])) && chrom_wanted(S, S->plan[c].name)) {
            R->pidx[R->n_plan] = c;
            R->plan[R->n_plan++] = &S->plan[c];
        }
    pd_set_walk(R->pd, S->P.one_base_rd_len / 4 + 1, S->P.overlap_mult, S->P.insert_max_size, R->keep);
    R->qord = R->pidx + n1;
    R->qpos = R->qord + n1;
    R->qplan = R->plan + n1;
    for (int k = 0; k < R->n_plan; k++) R->qord[k] = k;
    if (pd_device_mode(R->pd)) longest_first(R->qord, R->n_plan, R->plan);
    for (int q = 0; q < R->n_plan; q++) {
        R->qpos[R->qord[q]] = q;
        R->qplan[q] = R->plan[R->qord[q]];
    }
    /* the scan contexts get the run's insert parameters; the rows' file is opened */
    if (R->status) return 1; /* (the contexts could not be made) */
    for (int d = 0; d < S->n_init; d++)
        if (grom_ctx_set_params(d, &S->P) != GROM_OK) return 1;
    R->t_ctx = clock_gettime_s();
    R->pool.vcf = open_rows(S);
    return R->pool.vcf == NULL;
}

/* phase 4: the FASTA loaders (GROM_FASTA_THREADS, default 3; the device
 * loader is fed by one), working ahead of the hand-over in queue order */
static int streamed_feed_start(streamed_run *R) {
    cli_state *S = R->S;
    fasta_feed *F = &R->F;
    F->S = S;
    F->plan = R->qplan;
    F->n_plan = S->env.plan_only ? 0 : R->n_plan;
    F->ahead = 4;
    F->done = calloc((size_t)(R->n_plan > 0 ? R->n_plan : 1), 1);
    pthread_mutex_init(&F->mu, NULL);
    pthread_cond_init(&F->cv, NULL);
    const int want = S->fdev ? 1 : S->env.fasta_threads;
    while (F->n_thr < want && pthread_create(&F->thr[F->n_thr], NULL, fasta_main, F) == 0) F->n_thr++;
    if (F->n_thr == 0) fprintf(stderr, "grom: no FASTA loader thread\n");
    return F->n_thr == 0;
}

/* (references loaded but never handed to a worker are freed with the plan at
 * the end of cli_run, after the workers are joined; a worker frees its own
 * job's reference when its scan ends) */
static void streamed_feed_stop(fasta_feed *F) {
    if (!F->done) return;
    pthread_mutex_lock(&F->mu);
    F->stop = 1;
    pthread_cond_broadcast(&F->cv);
    pthread_mutex_unlock(&F->mu);
    for (int t = 0; t < F->n_thr; t++) pthread_join(F->thr[t], NULL);
    pthread_mutex_destroy(&F->mu);
    pthread_cond_destroy(&F->cv);
    free(F->done);
}

/* phase 5: every chromosome of the queue, once the decoder has staged it and
 * its reference is loaded, goes to the scan workers; rows that are ready are
 * written meanwhile.  (Plan-only: the workers print each chromosome's plan
 * line, so the host tests run the pool beside the streamed decoder) */
static void streamed_hand_over(streamed_run *R) {
    cli_state *S = R->S;
    fasta_feed *F = &R->F;
    grom_pool *pool = &R->pool;
    pool_start(pool, S, R->n_plan);
    pool->pos = R->qpos;
    for (int q = 0; q < R->n_plan; q++) {
        chrom_plan *c = R->qplan[q];
        const int cand = R->pidx[R->qord[q]];
        grom_stage *st = NULL;
        pd_chrom_facts facts;
        const int rc = pd_wait_chrom(R->pd, cand, &st, &facts);
        if (rc == 1) { R->fallback = 1; break; }
        if (rc != 0) {
            fprintf(stderr, "grom: streamed decode failed: %s\n", pd_error(R->pd));
            grom_set_last_error(pd_error(R->pd));
            R->status = 1;
            break;
        }
        if (!S->env.plan_only) {
            pthread_mutex_lock(&F->mu);
            while (F->loaded <= q) pthread_cond_wait(&F->cv, &F->mu);
            F->consumed = q + 1;
            pthread_cond_broadcast(&F->cv);
            pthread_mutex_unlock(&F->mu);
            /* the device loader's bytes go stage-ward device-to-device (same GPU), else from the host copy */
            const int d2d = c->ref && c->d_ref && R->dev_of[cand] == S->device;
            if (!c->ref || (d2d ? grom_stage_set_ref_device(st, c->d_ref, c->len)
                                : grom_stage_set_ref(st, c->ref, c->len)) != GROM_OK) {
                fprintf(stderr, "grom: staging the reference of %s failed: %s\n", c->name, grom_last_error());
                R->status = 1;
                pd_release_stage(R->pd, st);
                break;
            }
        }
        pthread_mutex_lock(&pool->mu);
        grom_job *j = &pool->jobs[q];
        j->cp = c;
        j->stage = st;
        j->facts = facts;
        j->pd = R->pd;
        j->k = cand;
        j->device = R->dev_of[cand];
        pd_trace(R->pd, PD_EV_HANDED, cand, 0);
        j->ready = 1;
        pthread_cond_broadcast(&pool->cv);
        drain_rows(pool, R->n_plan);
        pthread_mutex_unlock(&pool->mu);
    }
}

/* phase 6 (GROM_VERBOSE): the phases' times and the decoder's counters; bench.py reads these lines */
static void streamed_report(const streamed_run *R) {
    const cli_state *S = R->S;
    const double t_end = clock_gettime_s();
    printf("cli phases (s from start): candidates/FASTA lengths %.3f, decoder open %.3f, insert statistics %.3f, "
           "contexts %.3f, last chromosome handed %.3f, scans done %.3f; process start to CLI start %.3f\n",
           S->t_cand - S->t_cli0, R->t_started - S->t_cli0, R->t_stats - S->t_cli0, R->t_ctx - S->t_cli0,
           R->t_loop - S->t_cli0, t_end - S->t_cli0, S->t_load);
    pd_counters pc;
    pd_get_counters(R->pd, &pc);
    if (pc.device)
        printf("device decode: %lld records, %.2f GB compressed read and copied to HBM, %.2f GB inflated on the GPU; "
               "file reads %.2f s (read ahead; waited for %.2f s), device work %.2f s (GPU inflate %.3f s, record walk %.3f s, "
               "parse %.3f s; %lld of %lld walk sub-chunks re-walked), device buffer growth %.3f s, per-chromosome decode + "
               "finalise %.2f s, idle stage blocks reclaimed %lld, %d decode workers, %lld statistics-only runs, wall %.2f s\n",
               (long long)pc.records, pc.compressed_bytes / 1e9, pc.inflated_bytes / 1e9, pc.io_s, pc.wait_s,
               pc.decode_thread_s,
               pc.gpu_ms[0] / 1e3, pc.gpu_ms[1] / 1e3, pc.gpu_ms[2] / 1e3, (long long)pc.rewalked, (long long)pc.subchunks,
               pc.gpu_ms[3] / 1e3, pc.upload_s, (long long)pc.reclaimed, pc.dd_workers, (long long)pc.stats_only_runs,
               clock_gettime_s() - R->t_start);
    else
        printf("streamed decode: %lld records in %lld pieces, %d threads (%s), %.2f GB inflated, %.2f GB to HBM, "
               "decoder busy %.2f s (inflate %.2f s, file reads %.2f s), uploader %.2f s (waiting %.2f s), wall %.2f s\n",
               (long long)pc.records, (long long)pc.pieces, pc.threads, pc.libdeflate ? "libdeflate" : "zlib",
               pc.inflated_bytes / 1e9, pc.h2d_bytes / 1e9, pc.decode_thread_s, pc.inflate_s, pc.io_s, pc.upload_s, pc.wait_s,
               clock_gettime_s() - R->t_start);
    if (pc.verify_crc && pc.device) /* (a line of its own: the lines above keep their form) */
        printf("block checksums: every BGZF block's CRC-32 checked on the GPU, %.3f s (HIP events) next to the inflate's %.3f s\n",
               pc.crc_ms / 1e3, pc.gpu_ms[0] / 1e3);
    else if (pc.verify_crc)
        printf("block checksums: every BGZF block's CRC-32 checked by the decoder threads\n");
}

/* phase 7: the outputs, before any device memory is freed (that is teardown).
 * GROM_CLI_PROCESS=1 (opt-in, for a `grom` process; never for in-process
 * callers such as the Python binding): the process ends here */
static void streamed_outputs(streamed_run *R) {
    cli_state *S = R->S;
    const int good = !R->fallback && R->status == 0 && !bgzf_crc_error();
    S->t_scans = clock_gettime_s();
    if (R->pool.vcf) fclose(R->pool.vcf);
    if (good) finish_outputs(S, &R->pool.ctx_all);
    S->t_outputs = clock_gettime_s();
    if (!good || !S->env.cli_process || S->gz_failed) return;
    /* every scan has finished and the outputs are closed; the process's
     * device memory, streams and pinned buffers go with it (hipFree of
     * ~150 GB of stages and scratch, and the runtime's own teardown, are
     * 0.1-0.6 s of a whole run) */
    if (S->env.verbose)
        printf("cli teardown (s from start): scans done %.3f, outputs %.3f, process exit without freeing\n",
               S->t_scans - S->t_cli0, S->t_outputs - S->t_cli0);
    fflush(stdout);
    fflush(stderr);
    /* GROM_EXIT_HANDLERS=1: exit handlers still run (a profiler that
     * writes its records at exit, e.g. rocprofv3) */
    if (S->env.exit_handlers) exit(0);
    _exit(0);
}

/* phase 8, and every way out: the decoder closed, the stages freed, the
 * arrays released.  `rc`: an early phase's verdict, else the run's */
static int streamed_close(streamed_run *R, int rc) {
    cli_state *S = R->S;
    if (R->pd) pd_close(R->pd);
    S->t_decclose = clock_gettime_s();
    if (S->env.par_free && R->n_stages > 1) {
        /* (timing probe) the stages freed on threads of their own */
        pthread_t th[64];
        int started[64] = {0};
        for (int i = 0; i < R->n_stages && i < 64; i++)
            started[i] = pthread_create(&th[i], NULL, stage_free_main, R->stages[i]) == 0;
        for (int i = 0; i < R->n_stages; i++) {
            if (i < 64 && started[i]) pthread_join(th[i], NULL);
            else grom_stage_free(R->stages[i]);
        }
    } else {
        for (int i = 0; i < R->n_stages; i++) grom_stage_free(R->stages[i]);
    }
    S->t_pdclose = clock_gettime_s();
    free(R->pool.ctx_all.p);
    free(R->plan);
    free(R->dev_of);
    if (rc) return rc;
    if (R->fallback) {
        for (int d = 0; d < S->n_init; d++) grom_dev_fini(d);
        S->n_init = 0;
        return CLI_FALLBACK;
    }
    return R->status;
}

static int run_streamed(cli_state *S) {
    streamed_run run = {.S = S, .t_start = clock_gettime_s()}, *R = &run;
    int rc = streamed_open(R);
    /* the scan contexts while the head of the BAM is decoded (their insert
     * parameters are set once the statistics are known) */
    if (!rc) R->status = setup_workers(S) != 0;
    if (!rc) rc = streamed_insert_stats(R);
    if (!rc) { /* from here on a failure is the run's status, and its times are reported */
        if (streamed_plan(R) || streamed_feed_start(R)) R->status = 1;
        else streamed_hand_over(R);
        streamed_feed_stop(&R->F);
        R->t_loop = clock_gettime_s();
        if (R->pool.jobs) pool_finish(&R->pool);
        if (R->pool.status) R->status = 1;
        if (!R->fallback && R->status == 0 && S->env.verbose) streamed_report(R);
        streamed_outputs(R);
    }
    return streamed_close(R, rc);
}

/* A fatal signal prints the host stack before the process ends (addresses
 * resolve with addr2line against libgrom_amd.so): the grom executable's
 * handler (`abrt`: SIGABRT too), and with GROM_SEGV_TRACE=1 that of in-process
 * callers such as the Python binding, which have none */
static void on_fatal_trace(int sig) {
    void *fr[64];
    const int n = backtrace(fr, 64);
    static const char msg[] = "grom: fatal signal, host stack:\n";
    if (write(2, msg, sizeof(msg) - 1) < 0) { /* nothing more to do */ }
    backtrace_symbols_fd(fr, n, 2);
    signal(sig, SIG_DFL);
    raise(sig);
}

void cli_trace_fatal_signals(int abrt) {
    struct sigaction sa = {.sa_handler = on_fatal_trace};
    sigaction(SIGBUS, &sa, NULL);
    sigaction(SIGSEGV, &sa, NULL);
    if (abrt) sigaction(SIGABRT, &sa, NULL);
}

/* 1 if a file stands where the BAM's index is looked for (<bam>.bai or
 * <stem>.bai), readable or not */
static int index_file_present(const char *bam_path) {
    char path[4096];
    snprintf(path, sizeof(path), "%s.bai", bam_path);
    if (access(path, F_OK) == 0) return 1;
    const size_t n = strlen(bam_path);
    if (n > 4 && strcmp(bam_path + n - 4, ".bam") == 0) {
        snprintf(path, sizeof(path), "%.*s.bai", (int)(n - 4), bam_path);
        if (access(path, F_OK) == 0) return 1;
    }
    return 0;
}

/* phase: the options into the state (getopt string of GROM.c:21908).
 * -1: go on; else the exit code (-h, a bad option) */
static int cli_parse(cli_state *S, int argc, char **argv) {
    grom_params *P = &S->P;
    grom_default_params(P);
    S->max_chr_len = 300000000; /* g_max_chr_fasta_len, GROM.c:946 */
    S->num_sd = 3;
    S->n_dev = 1;
    S->one_chrom = -1;
    S->sub_end = 300000000; /* MAX_REGION, GROM.c:78 */
    S->device = S->env.device;
    optind = 0; /* GNU getopt: 0 fully re-initialises, so this is callable again */
    int opt;
    while ((opt = getopt(argc, argv,
                         "Z:W:X:Q:A:Y:B:D:E:K:N:V:U:L:F:SP:c:R:MG:i:r:o:p:q:s:v:g:l:d:b:n:a:y:z:e:fj:k:m:u:w:x:h")) != -1) {
        switch (opt) {
        case 'S': P->splitread = 0; break;
        case 'G': P->sv_list_len = atoi(optarg); break;
        case 'M': P->rmdup = 1; break;
        case 'i': S->bam_name = optarg; break;
        case 'r': S->fasta_name = optarg; break;
        case 'o': S->out_name = S->side_base = optarg; break;
        case 'B': S->max_chr_len = atol(optarg); break;
        case 'p': P->ploidy = atoi(optarg); break;
        case 'q': P->min_mapq = atoi(optarg); break;
        case 's': S->num_sd = atof(optarg); break;
        case 'g': P->gender = atoi(optarg); break;
        case 'l': P->overlap_mult = atoi(optarg); break;
        case 'b': P->min_base_qual = atoi(optarg); break;
        case 'n': P->min_snv = atoi(optarg); break;
        case 'a': P->min_snv_ratio = atof(optarg); break;
        case 'f': P->vcf = 0; break;
        case 'x': P->min_ave_bq = atof(optarg); break;
        case 'c':
            if (sscanf(optarg, "%d,%d,%d,%d", &S->one_chrom, &S->sub_child, &S->sub_start, &S->sub_end) < 1)
                S->one_chrom = -1;
            break;
        case 'P': { /* -P processes -> GPUs; 0 or beyond 256: serial, one GPU (GROM.c:21923-21927) */
            const int n = atoi(optarg);
            S->fetch = n >= 1 && n <= 256 && !S->env.p_serial;
            S->n_dev = n >= 1 && n <= 256 ? n : 1;
            break;
        }
        case 'Z': P->block_min = atol(optarg); break;
        case 'W': P->min_rd_window_len = atol(optarg); break;
        case 'X': P->max_rd_window_len = atol(optarg); break;
        case 'A': P->windows_sampling_factor = atol(optarg); break;
        case 'Y': P->min_blocks = atol(optarg); break;
        case 'D': P->min_repeat = atol(optarg); break;
        case 'E': P->min_repeat_stdev = atof(optarg); break;
        case 'K': P->ranks_stdev = atoi(optarg); break;
        case 'V': P->rd_pval_threshold = atof(optarg); break;
        case 'U': P->chr_rd_threshold_factor = atoi(optarg); break;
        case 'L': P->dup_threshold_factor = atol(optarg); break;
        case 'F': P->mapq_factor = atof(optarg); break;
        case 'v': P->pval_threshold = atof(optarg); break;
        case 'd': P->min_disc = atoi(optarg); break;
        case 'y': P->max_split_loss = atoi(optarg); break;
        case 'z': P->min_sr_len = atoi(optarg); break;
        case 'e': P->pval_insertion = atof(optarg); break;
        case 'j': P->min_sv_ratio = atof(optarg); break;
        case 'k': P->max_homopolymer = atoi(optarg); break;
        case 'm': P->min_indel_ratio = atof(optarg); break;
        case 'u': P->max_evidence_ratio = atof(optarg); break;
        case 'w': P->max_ins_range = atoi(optarg); break;
        case 'N': P->gen1000_window = atol(optarg); break;
        case 'h': print_help(); return 0;
        case '?': return 1;
        default: break; /* accepted; steers rows outside the implemented scan */
        }
    }
    P->rd_min_mapq = P->min_mapq;         /* GROM.c:22102 */
    P->pval_threshold1 = P->pval_threshold; /* GROM.c:22101 */
    P->sv_list2_len = P->sv_list_len / 10;  /* GROM.c:21925 */
    if (!S->force_serial) {
        printf("bam %s\n", S->bam_name ? S->bam_name : "(null)");
        printf("ref %s\n", S->fasta_name ? S->fasta_name : "(null)");
        printf("results %s\n", S->out_name ? S->out_name : "(null)");
    }
    if (!S->bam_name) { printf("ERROR: No bam file specified.\n"); return 1; }
    return -1;
}

/* phase: the BAM's header and index, and the output's name checked.
 * GROM_BUILD_INDEX=1: a BAM with no index file gets one, built on the run's
 * device (grom_bai_build_device); a file that is there is never replaced */
static int cli_open_bam(cli_state *S) {
    bgzf_reader br;
    const int bad = bgzf_open_read(&br, S->bam_name) != 0 || bam_read_header(&br, &S->hdr) != 0;
    bgzf_close_read(&br);
    if (bad) { printf("\nCould not open %s\n", S->bam_name); return 1; }
    if (S->env.build_index && !index_file_present(S->bam_name)) {
        int64_t bo[8];
        if (grom_bai_build_device(S->bam_name, NULL, S->device, bo) != 0) {
            printf("Could not build the BAM index: %s\n", grom_last_error());
            return 1;
        }
        printf("built %s.bai on device %d in %.3f s (%lld records, %.3f s on the device)\n", S->bam_name, S->device,
               (double)bo[7] / 1e6, (long long)bo[0], (double)bo[6] / 1e6);
    }
    if (!bai_loads(S->bam_name)) { printf("Could not open BAM indexing file\n"); return 1; }
    if (!S->out_name) { printf("ERROR: No output file specified.\n"); return 1; }
    if (S->one_chrom >= 0) {
        if (S->one_chrom >= S->hdr.n_ref) { printf("ERROR: -c %d: the BAM has %d targets\n", S->one_chrom, S->hdr.n_ref); return 1; }
        if (S->sub_start != 0) {
            printf("ERROR: -c with a sub-region (start %d): only whole-chromosome children are supported (-R is not)\n",
                   S->sub_start);
            return 1;
        }
        S->fetch = 1; /* g_parallel_mode = 1, GROM.c:22104 */
        snprintf(S->part_name, sizeof(S->part_name), "%s.%s-%d", S->out_name, S->hdr.ref_name[S->one_chrom], S->sub_child);
        S->out_name = S->part_name;
    } else {
        /* (GROM_VCF_BGZF: the plain file is never created) */
        snprintf(S->gz_name, sizeof(S->gz_name), "%s.gz", S->out_name);
        const char *name = S->env.vcf_bgzf ? S->gz_name : S->out_name;
        FILE *probe = fopen(name, "w");
        if (!probe) { printf("\nCould not open %s\n", name); return 1; }
        fclose(probe);
    }
    return 0;
}

/* phase: -r opened; then, beside what follows, the HIP start-up, the
 * footprint sampler (GROM_VERBOSE) and the tables (read_binom_tables,
 * GROM.c:22234) on threads of their own */
static int cli_open_fasta(cli_state *S, fp_sampler *fps) {
    if (!S->fasta_name) { printf("ERROR: No reference file specified.\n"); return 1; }
    if (cli_fasta_open(S) != 0) {
        memset(&S->fa, 0, sizeof(S->fa)); /* (what a failed open leaves is not for grom_fasta_close) */
        return 1;
    }
    if (!S->env.plan_only && !S->hip_started && !S->hip_done) hip_start(S);
    if (!S->env.plan_only && S->env.verbose) fp_start(fps, S->device);
    const size_t tn = (size_t)(GROM_MAX_TRIALS + 1) * (GROM_MAX_TRIALS + 1);
    S->hez = malloc(sizeof(double) * tn);
    S->mq = malloc(sizeof(double) * tn);
    S->tables_started = pthread_create(&S->tables_thr, NULL, tables_main, S) == 0;
    if (!S->tables_started) grom_build_tables(S->P.min_mapq, S->hez, S->mq);
    return 0;
}

/* the loader's length of every matched FASTA entry (find_disc_svs loads each
 * chromosome, GROM.c:21009-21045), several entries at once: fi_len[entry] */
static void fasta_lengths(cli_state *S, const int *fi_list, int n_fi, long *fi_len) {
    if (S->fdev) {
        /* the index pass measured them; a table adopted from .info: a length-only load each */
        for (int a = 0; a < n_fi; a++) {
            int64_t L = grom_fasta_dev_load(S->fdev, fi_list[a], NULL, 0, NULL);
            if (L < 0) L = cli_fasta_host_load(S, fi_list[a], NULL, 0);
            fi_len[fi_list[a]] = (long)L;
        }
        return;
    }
    long *lens = calloc(n_fi > 0 ? n_fi : 1, sizeof(long));
    const int thr = host_cpus() < 16 ? host_cpus() : 16;
    const int ok = !S->env.fasta_serial && grom_fasta_lengths(&S->fa, fi_list, n_fi, lens, thr) == 0;
    for (int a = 0; a < n_fi; a++) fi_len[fi_list[a]] = ok ? lens[a] : grom_fasta_load(&S->fa, fi_list[a], NULL, 0);
    free(lens);
}

/* phase: the candidate chromosomes in BAM header order (GROM.c:20826-21050);
 * the length test that needs the insert size comes later */
static int cli_candidates(cli_state *S) {
    const int n1 = S->hdr.n_ref > 0 ? S->hdr.n_ref : 1;
    S->plan = calloc(n1, sizeof(chrom_plan));
    int *fi_of = malloc(sizeof(int) * n1);   /* target -> FASTA entry, -1: none */
    int *fi_list = malloc(sizeof(int) * n1); /* the distinct entries */
    long *fi_len = calloc(S->fa.n > 0 ? S->fa.n : 1, sizeof(long));
    int n_fi = 0, rc = 0;
    for (int t = 0; t < S->hdr.n_ref; t++) {
        if (S->one_chrom >= 0 && t != S->one_chrom) { /* -c: loop_start = g_one_chromosome, GROM.c:20821 */
            fi_of[t] = -1;
            continue;
        }
        int fi = grom_match_target(&S->fa, S->hdr.ref_name[t]);
        char lc[GROM_MAX_CHR_NAMES];
        int bl = grom_target_name_lc(S->hdr.ref_name[t], lc, (int)sizeof(lc));
        if (S->P.gender == 0 && ((bl == 4 && strncmp(lc, "chry", 4) == 0) || (bl == 1 && lc[0] == 'y'))) fi = -1;
        fi_of[t] = fi;
        if (fi < 0) continue;
        int seen = 0;
        for (int a = 0; a < n_fi && !seen; a++) seen = fi_list[a] == fi;
        if (!seen) fi_list[n_fi++] = fi;
    }
    fasta_lengths(S, fi_list, n_fi, fi_len);
    for (int t = 0; t < S->hdr.n_ref && rc == 0; t++) {
        const int fi = fi_of[t];
        if (fi < 0) continue;
        long len = fi_len[fi];
        if (S->one_chrom >= 0 && len > S->sub_end) {
            printf("ERROR: -c region end %d is inside the chromosome (%ld bases): -R sub-regions are not supported\n",
                   S->sub_end, len);
            rc = 1;
            continue;
        }
        /* count_discordant_pairs re-derives the BAM target from the FASTA name
         * (GROM.c:1894-1961): the first target matching it */
        int32_t tid2 = -1;
        for (int a = 0; a < S->hdr.n_ref; a++)
            if (grom_match_target(&S->fa, S->hdr.ref_name[a]) == fi) { tid2 = a; break; }
        chrom_plan *c = &S->plan[S->n_cand++];
        c->fasta_idx = fi;
        c->tid = tid2;
        c->len = len;
        /* the name loop leaves the last target's name when nothing matches */
        c->target = strdup(S->hdr.n_ref > 0 ? S->hdr.ref_name[tid2 >= 0 ? tid2 : S->hdr.n_ref - 1] : "");
        snprintf(c->name, sizeof(c->name), "%.*s", S->fa.name_len[fi], S->fa.names[fi]);
    }
    free(fi_of);
    free(fi_list);
    free(fi_len);
    S->t_cand = clock_gettime_s();
    return rc;
}

/* phase: the CTX file's name, after the rows' (-c: the child's partial CTX file, GROM.c:20686) */
static void cli_name_outputs(cli_state *S) {
    const size_t ol = strlen(S->out_name);
    if (S->one_chrom < 0 && ol > 4 && strcmp(S->out_name + ol - 4, ".vcf") == 0)
        snprintf(S->ctx_name, sizeof(S->ctx_name), "%.*s.ctx.vcf", (int)(ol - 4), S->out_name);
    else
        snprintf(S->ctx_name, sizeof(S->ctx_name), "%s.ctx", S->out_name);
    snprintf(S->ctx_gz_name, sizeof(S->ctx_gz_name), "%s.gz", S->ctx_name);
}

/* phase (GROM_VERBOSE): the device FASTA loader's times, the teardown's, the footprint */
static void cli_report(cli_state *S, fp_sampler *fps) {
    if (S->fdev && S->env.verbose) {
        double ms[8];
        grom_fasta_dev_times(S->fdev, ms);
        fprintf(stderr, "grom: device FASTA loader (%s, device %d): file read + upload %.1f ms, inflate %.1f ms, index pass "
                        "kernels %.1f ms, load kernels %.1f ms, copies to the host %.1f ms; wall: open %.1f ms, index %.1f ms, "
                        "loads %.1f ms\n", grom_fasta_dev_is_bgzf(S->fdev) ? "BGZF" : grom_fasta_dev_kind(S->fdev) == 2 ? "gzip" : "plain text",
                S->device, ms[0], ms[1], ms[2], ms[3], ms[4], ms[5], ms[6], ms[7]);
        if (grom_fasta_dev_kind(S->fdev) == 2) {
            int64_t gs[8];
            double gm[6];
            grom_fasta_dev_gzip_stats(S->fdev, gs, gm);
            fprintf(stderr, "grom: gzip on the device: %lld units (%lld from guesses, %lld decoded again) in %lld members, "
                            "%lld marker bytes, scratch %.1f MB; guess %.1f ms, count %.1f ms, symbols %.1f ms, hand-over "
                            "%.1f ms, resolve %.1f ms, CRC %.1f ms\n", (long long)gs[0], (long long)gs[1], (long long)gs[2],
                    (long long)gs[4], (long long)gs[3], gs[6] / 1048576.0, gm[0], gm[1], gm[2], gm[3], gm[4], gm[5]);
        }
    }
    for (int d = 0; d < S->n_init; d++) grom_dev_fini(d);
    if (S->env.verbose && S->t_outputs > 0)
        printf("cli teardown (s from start): scans done %.3f, outputs %.3f, decoder closed %.3f, stages freed %.3f, "
               "contexts freed %.3f\n", S->t_scans - S->t_cli0, S->t_outputs - S->t_cli0, S->t_decclose - S->t_cli0,
               S->t_pdclose - S->t_cli0, clock_gettime_s() - S->t_cli0);
    fp_stop(fps, clock_gettime_s() - S->t_cli0);
}

/* phase: whatever the run made is released */
static void cli_release(cli_state *S, fp_sampler *fps) {
    tables_join(S);
    hip_ready(S);
    fp_stop(fps, -1.0); /* (a run that ended before its report: no line) */
    for (int i = 0; i < S->n_cand; i++) {
        free(S->plan[i].target);
        free(S->plan[i].ref);
        plan_release_dref(S, &S->plan[i]);
    }
    free(S->plan);
    free(S->hez);
    free(S->mq);
    free(S->vcf_segs.p);
    grom_fasta_close(&S->fa);
    grom_fasta_dev_close(S->fdev);
    dd_ctx_drop_prepared();
    bam_free_header(&S->hdr);
}

static int cli_run(int argc, char **argv, int force_serial, int *insert_printed) {
    cli_state *S = calloc(1, sizeof(cli_state));
    cli_settings_read(&S->env); /* on every call: in-process callers change the environment between runs */
    S->insert_printed = insert_printed;
    S->force_serial = force_serial;
    pthread_mutex_init(&S->fdev_mu, NULL);
    if (S->env.segv_trace) cli_trace_fatal_signals(0);
    setlinebuf(stdout);
    if (force_serial && S->env.verbose) printf("reading the BAM serially\n");
    S->t_cli0 = clock_gettime_s();
    S->t_load = since_process_start();
    fp_sampler fps = {0};
    int ret = cli_parse(S, argc, argv);
    if (ret < 0 && S->env.vcf_tabix && (S->one_chrom >= 0 || S->env.vcf_segs || S->P.vcf != 1)) {
        /* a child's rows have no header, the segments are byte ranges of the unsorted file, tab rows are not VCF */
        printf("ERROR: GROM_VCF_TABIX cannot be combined with %s\n",
               S->one_chrom >= 0 ? "-c (a -P child): its rows are a part of a file"
               : S->env.vcf_segs ? "GROM_VCF_SEGS: the rows' byte offsets are those of the plain, unsorted file"
                                 : "-f: tab-separated rows are not VCF");
        ret = 1;
    } else if (ret < 0 && S->env.vcf_bgzf && (S->one_chrom >= 0 || S->env.vcf_segs)) {
        /* both depend on plain byte offsets in the rows' file; refused before any file or device is touched */
        printf("ERROR: GROM_VCF_BGZF cannot be combined with %s: the rows' byte offsets are those of the plain file\n",
               S->one_chrom >= 0 ? "-c (a -P child)" : "GROM_VCF_SEGS");
        ret = 1;
    } else if (ret < 0) {
        ret = 1;
        if (cli_open_bam(S) == 0 && cli_open_fasta(S, &fps) == 0 && cli_candidates(S) == 0) {
            cli_name_outputs(S);
            ret = reads_serially(S) ? run_serial(S) : run_streamed(S);
            cli_report(S, &fps);
            if (S->gz_failed && ret == 0) ret = 1;
        }
        cli_release(S, &fps);
    }
    pthread_mutex_destroy(&S->fdev_mu);
    free(S);
    return ret;
}

int grom_cli_main(int argc, char **argv) {
    int insert_printed = 0;
    bgzf_crc_error_clear();
    int rc = cli_run(argc, argv, 0, &insert_printed);
    /* the streamed path could not be used -- but never after a block failed
     * its CRC-32: the serial reader would meet the same bytes */
    if (rc == CLI_FALLBACK && !bgzf_crc_error()) rc = cli_run(argc, argv, 1, &insert_printed);
    if (bgzf_crc_error()) { /* (a reader's loop may have taken the error for the end of the file) */
        fprintf(stderr, "grom: %s\n", bgzf_crc_error());
        grom_set_last_error(bgzf_crc_error());
        if (rc == 0 || rc == CLI_FALLBACK) rc = 1;
    }
    return rc;
}
