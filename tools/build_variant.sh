#!/bin/bash
# build an A/B variant of the library into ab_libs/: tools/build_variant.sh NAME "-DMACRO ..." [file.hip ...]
# (objects of the listed files are rebuilt with the extra flags, the rest are taken from csrc/)
set -e
NAME=$1; FLAGS=$2; shift 2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CS=$ROOT/distributed-multi-agent-slam-swarm-robotics-system_amd/csrc
mkdir -p $ROOT/ab_libs /tmp/abobj_$NAME
OBJS=""
SRCS=$(sed -n 's/^SRCS := //p' $CS/Makefile)     # the library's sources, as the Makefile lists them
for f in ${SRCS//.hip/}; do
  if [[ " $* " == *" $f.hip "* ]]; then
    EXTRA=""; [[ $f == icp ]] && EXTRA="-mllvm -amdgpu-mfma-vgpr-form=1"     # (the Makefile's per-file flag)
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math $EXTRA $FLAGS -c $CS/$f.hip -o /tmp/abobj_$NAME/$f.o
    OBJS="$OBJS /tmp/abobj_$NAME/$f.o"
  else
    OBJS="$OBJS $CS/$f.o"
  fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $ROOT/ab_libs/$NAME.so $OBJS -ldl
echo built ab_libs/$NAME.so
