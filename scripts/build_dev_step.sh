#!/bin/bash
# Dev variants of the whole libquadswarm.so (step kernels included):
#   build_dev_step.sh NAME "HIPCC FLAGS"   -> build/dev/lib_NAME.so (QS_DEV_LIB=<path> selects it)
# e.g. build_dev_step.sh floor "-DQS_X_NOCOMPUTE" (the probes: csrc/step_kernel_dev.h)
# The units are the Makefile's SRCS.  Variants that differ in one unit only (QS_RING_ITEMS
# touches step_mh_ring alone) need not compile the rest again:
#   KEEP_OBJS=1 build_dev_step.sh floor "-DQS_X_NOCOMPUTE"                 keeps build/dev/floor/*.o
#   FROM=floor UNITS=step_mh_ring build_dev_step.sh floor_nohist "-DQS_X_NOCOMPUTE -DQS_RING_ITEMS=0"
# compiles UNITS with the flags given and links them with the kept objects of FROM.
set -eu
cd "$(dirname "$0")/../marl-gym-pybullet-drones_amd"
name=$1; extra=$2
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-hip-fp32-correctly-rounded-divide-sqrt -fno-slp-vectorize -I../include -DQS_DEV_BUILD $extra"
all=$(sed -n 's/^SRCS *= *//p' Makefile | tr ' ' '\n' | sed -n 's#^csrc/\(.*\)\.hip$#\1#p')
[ -n "$all" ] || { echo "no SRCS in the Makefile" >&2; exit 1; }
units=${UNITS:-$all}
mkdir -p build/dev/$name
if [ -n "${FROM:-}" ]; then
  for u in $all; do cp build/dev/$FROM/$u.o build/dev/$name/$u.o; done
fi
pids=""
for u in $units; do
  /opt/rocm/bin/hipcc $FLAGS -c -o build/dev/$name/$u.o csrc/$u.hip &
  pids="$pids $!"
done
for p in $pids; do wait $p; done
objs=""
for u in $all; do objs="$objs build/dev/$name/$u.o"; done
/opt/rocm/bin/hipcc $FLAGS -shared -o build/dev/lib_$name.so $objs
[ -n "${KEEP_OBJS:-}" ] || rm -rf build/dev/$name
echo "built build/dev/lib_$name.so"
