#!/bin/bash
# Build the k_tree phase-stamp diagnostic library (abv/ts/liboamd.so) for
# tools/tree_stamps.py (run on the GPU box by tools/gpu.sh "stamps NAME ts").
# The units and their flags are build.py's UNITS, as in tools/variants.sh.
set -eu
cd "$(dirname "$0")/.."
CS=othello-alphazero_amd/csrc
CXX="/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -fno-gpu-rdc -I $CS -I include -DOAMD_TREE_STAMPS"
# "unit flags..." per line (without the resource remarks build.py's checks read)
mapfile -t UNITS < <(python3 -c "
import sys
sys.path.insert(0, 'othello-alphazero_amd')
import build
for u, f in build.UNITS.items():
    print(u, *[x for x in f if not x.startswith('-Rpass')])")
mkdir -p abv/ts
pids=()
for u in "${UNITS[@]}"; do
  read -r unit uflags <<< "$u"
  $CXX $uflags -c $CS/$unit -o abv/ts/$unit.o &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o abv/ts/liboamd.so abv/ts/*.o
rm -f abv/ts/*.o
echo built abv/ts/liboamd.so
