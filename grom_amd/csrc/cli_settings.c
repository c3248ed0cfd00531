/* cli_settings.c -- the command line's GROM_* environment knobs: each one's
 * name, default and clamp, once.  Plain C, nothing but getenv. */
#include <stdlib.h>
#include <string.h>

#include "cli_settings.h"

static int is_set(const char *k) { return getenv(k) != NULL; }
static int num(const char *k, int unset) { const char *v = getenv(k); return v ? atoi(v) : unset; }
static int is_1(const char *k) { return num(k, 0) == 1; }
static int within(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

void cli_settings_read(cli_settings *s) {
    memset(s, 0, sizeof(*s));
    s->plan_only = is_set("GROM_PLAN_ONLY");        /* report the record plan, no GPU */
    s->verbose = is_set("GROM_VERBOSE");            /* phase times, counters, footprint */
    s->fasta_serial = is_set("GROM_FASTA_SERIAL");  /* FASTA lengths one entry at a time */
    s->segv_trace = is_set("GROM_SEGV_TRACE");      /* a fatal signal prints the host stack */
    s->no_warm = is_set("GROM_NO_WARM");            /* no device decoder warm-up at start */
    s->stage_digest = is_set("GROM_STAGE_DIGEST");  /* test hook: a digest line per staged chromosome */
    s->copy_stats = is_set("GROM_COPY_STATS");      /* grom: exit handlers run (they print the copy statistics) */
    s->no_ctx_prepare = is_1("GROM_NO_CTX_PREPARE"); /* the decode worker makes its own context */
    s->par_free = is_1("GROM_PAR_FREE");            /* timing probe: stages freed on threads */
    s->cli_process = is_1("GROM_CLI_PROCESS");      /* the process ends once the outputs are written */
    s->exit_handlers = is_1("GROM_EXIT_HANDLERS");  /* ... through exit(), for a profiler's handlers */
    s->p_serial = is_1("GROM_P_SERIAL");            /* -P n: the serial stream's input on n GPUs */
    s->serial_decode = num("GROM_SERIAL_DECODE", 0) > 0; /* the serial BAM reader */
    s->build_index = num("GROM_BUILD_INDEX", 0) != 0;    /* a missing BAM index is built on the device */
    s->vcf_bgzf = num("GROM_VCF_BGZF", 0) != 0;          /* the rows and the CTX file written as BGZF on the device */
    s->vcf_tabix = num("GROM_VCF_TABIX", 0) != 0;        /* ... position-sorted, with a tabix index (implies BGZF) */
    if (s->vcf_tabix) s->vcf_bgzf = 1;
    s->device_decode = num("GROM_DEVICE_DECODE", -1);    /* 0: BAM decode on host threads */
    s->fasta_device = num("GROM_FASTA_DEVICE", -1); /* 0: a BGZF -r on the host; 1: a plain -r on the device */
    s->dump = getenv("GROM_DUMP");                  /* test hook: counter dumps, named after this prefix */
    s->vcf_segs = getenv("GROM_VCF_SEGS");          /* file for each chromosome's byte range in the VCF */
    s->ctx_raw = getenv("GROM_CTX_RAW");            /* file for the raw CTX rows */
    s->chroms = getenv("GROM_CHROMS");              /* name[,name...]: scan only these */
    s->filedate = getenv("GROM_FILEDATE");          /* pins ##fileDate */
    s->has_seed = is_set("GROM_SEED");              /* pins every chromosome's sampling seed */
    if (s->has_seed) s->seed = (uint32_t)strtoul(getenv("GROM_SEED"), NULL, 10);
    s->device = num("GROM_DEVICE", 0);              /* the run's (first) GPU */
    s->devices = is_set("GROM_DEVICES") ? within(num("GROM_DEVICES", 0), 1, 1 << 30) : 0; /* GPUs, over -P */
    s->scans_per_gpu = within(num("GROM_SCANS_PER_GPU", 2), 1, 1 << 30);          /* scan contexts per GPU */
    s->stages = within(num("GROM_STAGES", s->scans_per_gpu), 1, 1 << 30);         /* staged inputs per GPU */
    s->fasta_threads = within(num("GROM_FASTA_THREADS", 3), 1, 8);                /* host FASTA loaders */
    s->has_decode_threads = is_set("GROM_DECODE_THREADS"); /* unset: 4 serial, min(CPUs, 32) streamed */
    s->decode_threads = num("GROM_DECODE_THREADS", 0);
    s->n_worker_devices = -1;                       /* test hook: one scan worker per listed device */
    const char *wd = getenv("GROM_WORKER_DEVICES");
    if (wd) {
        char *dup = strdup(wd), *save = NULL;
        s->n_worker_devices = 0;
        for (char *tok = strtok_r(dup, ",", &save); tok && s->n_worker_devices < CLI_MAX_WORKERS;
             tok = strtok_r(NULL, ",", &save))
            s->worker_devices[s->n_worker_devices++] = atoi(tok);
        free(dup);
    }
}
