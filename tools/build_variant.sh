#!/bin/bash
# tools/build_variant.sh NAME [-D...]: builds rpo_amd/build/ab/librpo_NAME.so with extra flags for gemm.hip
# (SRC=<file without .hip> picks another translation unit; other objects reused from the last `python -m rpo_amd.build`); load it with RPO_HIP_LIB=... for A/B runs.
# The library links the translation units of rpo_amd/build.py's SOURCES, so that _lib.load() finds every export it checks.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
name=$1; shift
mkdir -p $R/rpo_amd/build/ab
SRC=${SRC:-gemm}
units=$(cd $R && python -c "from rpo_amd.build import SOURCES; print(' '.join(s[:-len('.hip')] for s in SOURCES))")
extra=$(cd $R && python -c "from rpo_amd.build import EXTRA_FLAGS; print(' '.join(EXTRA_FLAGS.get('$SRC.hip', [])))")
case " $units " in *" $SRC "*) ;; *) echo "SRC=$SRC is not one of: $units" >&2; exit 1;; esac
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -Wno-unused-function $extra "$@" -c $R/rpo_amd/csrc/$SRC.hip -o $R/rpo_amd/build/ab/${SRC}_$name.o
objs=""
for o in $units; do
  if [ $o = $SRC ]; then objs="$objs $R/rpo_amd/build/ab/${SRC}_$name.o"; else objs="$objs $R/rpo_amd/build/$o.o"; fi
done
hipcc --offload-arch=gfx950 -shared -fPIC -Wl,--version-script=$R/rpo_amd/csrc/exports.map $objs -o $R/rpo_amd/build/ab/librpo_$name.so
echo built $name
