#!/bin/bash
# An experimental build of the library for A/B runs (scripts/ab_tiles.py): tools/build_variant.sh NAME "-DFLAG ..."
#   -> tools/_bin/libnbc_NAME.so (git-ignored, travels with gpurun)
set -e
cd "$(dirname "$0")/.."
name=$1; flags=$2; srcdir=${3:-neuralbarkcalculator_amd/csrc}     # third argument: another source directory (e.g. an older revision)
obj=tools/_bin/obj_$name; mkdir -p $obj
pids=
rm -f $obj/*.o                             # the link takes every object here: none of an earlier build under this name
for path in $srcdir/*.cpp $srcdir/*.hip; do   # whatever the directory holds (an older revision has other files)
  src=$(basename $path)
  extra="-ffp-contract=off"; case $src in *.hip) extra="-x hip";; esac
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function $flags $extra -Iinclude -c $path -o $obj/$src.o &
  pids="$pids $!"
done
for pid in $pids; do wait $pid; done       # a failed compile ends the script (a bare `wait` would link what is left;
                                           # the other compiles finish into $obj, which the next build empties first)
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o tools/_bin/libnbc_$name.so $obj/*.o
echo tools/_bin/libnbc_$name.so
