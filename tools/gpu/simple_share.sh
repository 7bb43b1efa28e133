#!/bin/bash
# Share of align_kernel<128>'s wave cycles taken by the reads that end with one element and one scored
# location (PHASE_TIMERS=2 build: MK='s/PHASE_TIMERS ?= 0/PHASE_TIMERS ?= 2/' tools/build_variant.sh simple2 ""):
# C2, or with `c3` the C3 genome, 1M reads -> <output directory>/simple_share_<c2|c3>.json
#   tools/gpu/simple_share.sh <output directory> [c2|c3]
export TMPDIR=/tmp SNAPGPU_TIMEOUT_S=120 SNAPGPU_PHASES=1 SNAPGPU_LIB=$PWD/snap-rnaseq_amd/snapgpu/libsnapgpu_simple2.so
O=${1:?output directory}; W=${2:-c2}; mkdir -p $O
EXTRA=""; [ "$W" = c3 ] && EXTRA="--genome-bases 3100000000 --contigs 25 --families 2000"
timeout -k 10 700 python tools/phase_probe.py --simple-share $EXTRA > $O/simple_share_$W.json 2> $O/simple_share_$W.err || { tail $O/simple_share_$W.err; exit 1; }
cat $O/simple_share_$W.json
