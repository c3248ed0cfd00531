/* grom_cli.c -- the `grom` executable: a thin wrapper over grom_cli_main.
 * A fatal signal prints the host stack (cli_trace_fatal_signals, grom_main.c)
 * before the process ends. */
#include <stdio.h>
#include <unistd.h>

#include "../../include/grom_amd.h"
#include "cli_settings.h"

int main(int argc, char **argv) {
    cli_trace_fatal_signals(1);
    /* GROM_CLI_PROCESS=1 (opt-in): the library ends the process once the
     * outputs are written instead of freeing its device memory.  Not the
     * default: the driver then releases ~150 GB after the exit, and the next
     * run's large allocations wait for it (3.7 s per stage in back-to-back
     * runs) -- the freeing is only moved, not saved */
    const int rc = grom_cli_main(argc, argv);
    /* Every output is closed and the library has freed its device memory by
     * now; what is left of a normal exit is the runtime's own teardown in its
     * exit handlers (~0.1-0.2 s).  The process ends without it unless a tool
     * needs the handlers: a profiler that writes its records at exit
     * (GROM_EXIT_HANDLERS=1, e.g. rocprofv3) or the copy statistics
     * (GROM_COPY_STATS). */
    cli_settings env; /* (read again here: the run's own record ended with it) */
    cli_settings_read(&env);
    if (!env.exit_handlers && !env.copy_stats) {
        fflush(stdout);
        fflush(stderr);
        _exit(rc);
    }
    return rc;
}
