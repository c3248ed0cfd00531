/* ctxpost.h -- the translocation post-pass (ctxpost.c) writing to a FILE, as the command line calls it */
#ifndef GROM_CTXPOST_H
#define GROM_CTXPOST_H
#include <stdio.h>
#include "bamio.h"
void ctx_postpass(const char *raw, size_t raw_len, const bam_hdr *hdr, int Mx, int glseq, int vcf, FILE *out);
#endif
