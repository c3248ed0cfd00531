#!/bin/bash
# tools/record_cnv_host.sh [outdir] -- on a machine with the GPU, from the
# repository root: record cnvcall.cpp's inputs and outputs from real GPU scans
# (GROM_CNV_HOST_DUMP) of CNV parity cases into outdir (default cnvh_records/,
# gzipped), one record per chromosome.  A record is kept
# only from a run whose rows equal the oracle's, so the recorded rows are the
# oracle's.  The records become tests/golden/cnvh_*.cnvh.gz, which
# tests/test_sanitize.py replays under ASan and TSan (san_driver cnvhost).
#   multi: cnv_multi -V 1 -p 3
#   draws: cnv -V 1 with GROM_SAMPLE_LISTS_LEN=40 (the reservoir draws fire;
#          the oracle reads the same variable)
#   repeat: a small two-contig genome with -V 1 -D 4 -E 0 -X 2000 (repeats from
#          4 bases and no stdev margin: a most biased repeat type exists, so
#          the repeat sampler and the z override run; the genome is small and
#          -X 2000 short because every repeat is gathered with its flanks)
set -o pipefail
out=${1:-cnvh_records}
mkdir -p $out
repo=$(pwd)
work=$(mktemp -d)
cd $work
export GROM_FILEDATE=20260101 GROM_SEED=7
$repo/grom_amd/bin/grom_synth -o cnv_multi -L 700000,900000 -s 17 -V 0.000005 -W 15000,80000 -Q 0.08 || exit 1
$repo/grom_amd/bin/grom_synth -o cnv_small -L 150000,110000 -s 27 -V 0.00003 -W 5000,20000 -Q 0.08 || exit 1
$repo/grom_amd/bin/grom_synth -o cnv -L 1500000 -s 16 -V 0.000004 -W 20000,150000 -Q 0.05 || exit 1
record() {  # tag, input, environment assignment, flags...
    local tag=$1 in=$2 envset=$3
    shift 3
    mkdir -p $tag
    env $envset GROM_CNV_HOST_DUMP=$tag timeout -k 10 120 $repo/grom_amd/bin/grom -i $in.bam -r $in.fa -o g_$tag.vcf "$@" > /dev/null || exit 1
    env $envset timeout -k 10 600 $repo/oracle/grom_oracle -i $in.bam -r $in.fa -o o_$tag.vcf "$@" > /dev/null || exit 1
    cmp g_$tag.vcf o_$tag.vcf || { echo "$tag: rows differ from the oracle's, nothing recorded"; exit 1; }
    for f in $tag/*.cnvh; do gzip -9 -c $f > $repo/$out/cnvh_${tag}.$(basename $f).gz; done
}
record multi cnv_multi GROM_SEED=7 -V 1 -p 3
record draws cnv GROM_SAMPLE_LISTS_LEN=40 -V 1
record repeat cnv_small GROM_SEED=7 -V 1 -D 4 -E 0 -X 2000
ls -la $repo/$out
rm -rf $work
