#!/bin/bash
# Build liboamd.so variants HERE (CPU container) for the GPU-box recipes
# `variants` / `benchvar` of tools/gpu.sh:
#   VARIANTS="name:extra flags[:SRC];name2:..." bash tools/variants.sh
# SRC: empty = the tree's resnet.hip with the tree's other objects; + =
# every unit of the working tree built with the flags;
# a path = that resnet.hip with the tree's other objects; @REV = all of
# csrc/ and include/ at git revision REV (capi_net.hip packs the weights, so a
# variant that changes the packing must bring its own C ABI units; the search
# tree is spread over several units and headers, so another tree is a revision
# too). The units and
# their flags are build.py's UNITS (resnet.hip's from RF). Built into
# abv/<name>/liboamd.so (the pybind layer binds the C ABI, not the variant).
set -eu
cd "$(dirname "$0")/.."
B=othello-alphazero_amd/build
CS=othello-alphazero_amd/csrc
RF=${RF-"-mllvm -amdgpu-mfma-vgpr-form=1 -mllvm -amdgpu-sched-strategy=max-ilp"}  # env RF overrides (scheduler A/Bs)
CXX="/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -fno-gpu-rdc"
# "unit flags..." per line, as build.py builds them (without the resource remarks its checks read)
mapfile -t UNITS < <(OAMD_RESNET_FLAGS="$RF" python3 -c "
import sys
sys.path.insert(0, 'othello-alphazero_amd')
import build
for u, f in build.UNITS.items():
    print(u, *[x for x in f if not x.startswith('-Rpass')])")
rm -rf abv
IFS=';' read -ra SETS <<< "${VARIANTS:?}"
pids=()
for e in "${SETS[@]}"; do
  IFS=':' read -r name flags src <<< "$e"
  mkdir -p abv/$name
  (
    set -e
    dir=$CS inc="-I $CS -I include" every=1 rflags=$flags resnet=
    case "${src:-}" in
      +) ;;                           # every unit of the working tree, built with the flags
      @*)                             # every unit at a revision (the flags: its resnet.hip only)
        dir=abv/$name/src/$CS inc="-I $dir -I abv/$name/src/include" flags=
        mkdir -p abv/$name/src
        git archive "${src#@}" $CS include | tar -x -C abv/$name/src ;;
      *) every=0 resnet=${src:-} ;;   # only resnet.hip (or the one given), the build's other objects
    esac
    objs=
    for u in "${UNITS[@]}"; do
      read -r unit uflags <<< "$u"
      s=$dir/$unit f=$flags
      if [[ $unit == resnet.hip ]]; then s=${resnet:-$s} f=$rflags
      elif [[ $every == 0 ]]; then objs+=" $B/$unit.o"; continue
      fi
      [[ -f $s ]] || continue  # a revision from before the unit existed
      $CXX $inc $f $uflags -c $s -o abv/$name/$unit.o
      objs+=" abv/$name/$unit.o"
    done
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o abv/$name/liboamd.so $objs
    rm -rf abv/$name/*.o abv/$name/src
    echo "built $name"
  ) &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
