/* cli_settings.h -- every GROM_* environment knob the command line (grom_main.c,
 * grom_cli.c) honours, read by cli_settings_read at the start of every run
 * (and by grom's main at its end, for how the process exits).  The knobs of
 * other files (pdecode.c, scan.hip, ddecode.hip, ...) are read where they are
 * used.  cli_settings.c lists each knob with its default and clamp. */
#ifndef GROM_CLI_SETTINGS_H
#define GROM_CLI_SETTINGS_H
#include <stdint.h>

#define CLI_MAX_WORKERS 64

typedef struct {
    /* set at all */
    int plan_only, verbose, fasta_serial, segv_trace, no_warm, stage_digest, copy_stats;
    /* set to 1 */
    int no_ctx_prepare, par_free, cli_process, exit_handlers, p_serial;
    int serial_decode;                /* set above 0 */
    int build_index;                  /* set and not 0 */
    int vcf_bgzf;                     /* set and not 0 */
    int vcf_tabix;                    /* set and not 0; sets vcf_bgzf */
    int device_decode, fasta_device;  /* -1 unset, else the number given (0 and 1 are tested) */
    /* the text given, NULL when unset */
    const char *dump, *vcf_segs, *ctx_raw, *chroms, *filedate;
    int has_seed;
    uint32_t seed;
    int device;                       /* 0 unset */
    int devices;                      /* 0 unset, else at least 1 */
    int scans_per_gpu, stages, fasta_threads;
    int has_decode_threads, decode_threads; /* as given; each reader has its own default */
    /* GROM_WORKER_DEVICES: n_worker_devices -1 unset, else the list's length (at most CLI_MAX_WORKERS) */
    int n_worker_devices, worker_devices[CLI_MAX_WORKERS];
} cli_settings;

void cli_settings_read(cli_settings *s);
void cli_trace_fatal_signals(int abrt); /* grom_main.c: a fatal signal prints the host stack */

#endif
