#!/bin/bash
# k_score_fm timing probes (GCR_PROBE bits; results invalid when set) and
# A/B builds (LIBS: in-tree libraries, e.g. "libgcr.so libgcr_x.so" from
# `make variant`): the live launch average per setting.
# usage: [PROBES="0 1 ..."] [LIBS="..."] tools/probe_fm.sh [outdir] [workload]
# The probe bits inside k_score_fm's round loops (1, 2, 4, 32, 64, 256, 512,
# 1024) are compiled in only with -DGCR_FM_PROBES: the default library here is
# that variant, libgcr_probes.so, built if it is not there yet (build it where
# the rest is built; a missing one is compiled on the spot).
set -u
O=${1:-gpurun_out/probe}; W=${2:-m2}; mkdir -p $O
R=$(cd "$(dirname "$0")/.." && pwd)
if [ -z "${LIBS:-}" ] && [ ! -f "$R/graph-cut-ransac_amd/pygcransac/libgcr_probes.so" ]; then
  make -C "$R/graph-cut-ransac_amd/csrc" -j16 variant NAME=probes DEFS=-DGCR_FM_PROBES > $O/probe_build.log 2>&1 || { tail -5 $O/probe_build.log; exit 1; }
fi
for lib in ${LIBS:-libgcr_probes.so}; do
for pb in ${PROBES:-0 1 2 3 64 0}; do
  tag=${lib%.so}_$pb
  GCR_LIB=$lib GCR_PROBE=$pb timeout -k 10 120 python -u bench.py --workload $W --steps 400 --warmup 20 --cpu-seconds 0 --no-latency --no-hbm-probe > $O/probe_$tag.log 2>&1 || { tail -5 $O/probe_$tag.log; exit 1; }
  python3 -c "
import json,sys; d=json.loads(open('$O/probe_$tag.log').read().strip().splitlines()[-1]); r=d['roofline']
print('$lib probe $pb', 'kernel_us %.2f' % (1e3*r['avg_kernel_ms']), 'step_ms %.4f' % d['ms_per_step'])"
done
done
