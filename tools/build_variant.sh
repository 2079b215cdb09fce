#!/bin/bash
# Usage: tools/build_variant.sh NAME "<extra -D flags>" [TU ...]
# Builds ldsr_amd/libldsr_hip_NAME.so for same-box A/B runs (tools/ab.sh): the listed translation
# units (default: em_scan_16_1 kernels_scan) are recompiled with the extra flags, every other
# object is taken from the normal build (run `make -C ldsr_amd/csrc` first).  A unit is named like
# its object: members of the EM kernel families are em_scan_<L>_<W> / em_pair_<L>_<LPC>
# (ldsr_amd/csrc/em_members.h), compiled from the two *_launch.inc bodies as the Makefile does.
set -e
name=$1; flags=$2; shift 2
tus=${@:-em_scan_16_1 kernels_scan}
cd "$(dirname "$0")/../ldsr_amd/csrc"
mkdir -p /tmp/ldsr_var_$name
objs=""
for o in *.o; do
  b=${o%.o}
  if echo " $tus " | grep -q " $b "; then
    case $b in
      em_scan_*) src="-DSCAN_L=$(echo $b | cut -d_ -f3) -DSCAN_W=$(echo $b | cut -d_ -f4) -x hip em_scan_launch.inc" ;;
      em_pair_*) src="-DPAIR_L=$(echo $b | cut -d_ -f3) -DPAIR_LPC=$(echo $b | cut -d_ -f4) -x hip em_pair_launch.inc" ;;
      *) src=$b.hip ;;
    esac
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --offload-compress --offload-compression-level=19 -Wall -Wno-unused-function $flags -c $src -o /tmp/ldsr_var_$name/$b.o &
    objs="$objs /tmp/ldsr_var_$name/$b.o"
  else
    objs="$objs $o"
  fi
done
wait
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 --offload-compress -o ../libldsr_hip_$name.so $objs
echo built ldsr_amd/libldsr_hip_$name.so
