#!/bin/bash
# tools/scratch_scan.sh [-a] [-u "UNIT ..."] [CSRC_DIR] : kernels of the library that use scratch memory (register spills or private
# arrays), per translation unit, compiled with the Makefile's flags for the unit (-Rpass-analysis=kernel-resource-usage).  A hot
# kernel that picks up spills after an unrelated change is a silent regression (round 5: the fused inverse pass, 28 bytes per lane,
# -15 %): run this after touching wgfft.h or a pass.
#   -a        every kernel with its VGPRs and scratch, not only the ones that use scratch (the register tables of profiles/HISTORY.md)
#   -u UNITS  these units only (default: UNITS of the Makefile)
ALL=0
UNITS=
while getopts "au:" o; do
  case $o in
    a) ALL=1 ;;
    u) UNITS=$OPTARG ;;
    *) echo "usage: $0 [-a] [-u \"UNIT ...\"] [CSRC_DIR]" >&2; exit 2 ;;
  esac
done
shift $((OPTIND - 1))
D=${1:-$(dirname "$0")/../dspsr_amd/csrc}
cd "$D" || exit 2
[ -n "$UNITS" ] || UNITS=$(sed -n 's/^UNITS *= *//p' Makefile)
T=$(mktemp -d)
for u in $UNITS; do
  [ -f $u.hip ] || continue
  s=$(grep "^SCHED_$u " Makefile | sed 's/^[^=]*= *//')
  ( /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=on $s -Rpass-analysis=kernel-resource-usage -c -o $T/$u.o $u.hip 2>&1 \
    | grep -E "Function Name|ScratchSize|    VGPRs:" | sed 's/ \[-Rpass-analysis=kernel-resource-usage\]//; s/^.*remark: *//' | paste - - - \
    | awk -F'\t' -v u=$u -v all=$ALL '{ split($3, a, ": "); split($2, b, ": "); split($1, c, ": "); if (all || a[2] + 0 > 0) printf "%-20s scratch %4d B/lane  VGPRs %3d  %s\n", u, a[2], b[2], c[2] }' \
    > $T/$u.txt ) &
done
wait
for u in $UNITS; do [ -f $T/$u.txt ] && cat $T/$u.txt; done
rm -rf $T
