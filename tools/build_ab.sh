#!/bin/bash
# (round 4 used an earlier form of this script for an A/B of sweep_lazy.hip alone: the history has it)
# build_ab.sh [commit] — the three libraries of a same-box A/B of the sweep (select each with PARTLS_LIB):
#   libpartls_hip.so             the working tree
#   libpartls_hip_parent.so      <commit> (default HEAD), built from an export of it in a temporary directory
#   libpartls_hip_parent_t16.so  the placement control: <commit>'s sources with sweep_blk.hip compiled for T = 16 alone (-DPARTLS_ONLY_T=16)
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
REV=${1:-HEAD}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="-O3 -fPIC -std=c++17 --offload-arch=gfx950 -Wall -Wno-unused-function -ffp-contract=off"
make -s -C "$ROOT/partitionedls.jl_amd/csrc" -j8
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
git -C "$ROOT" archive "$REV" | tar -x -C "$TMP"
make -s -C "$TMP/partitionedls.jl_amd/csrc" -j8
cp "$TMP/partitionedls.jl_amd/libpartls_hip.so" "$ROOT/partitionedls.jl_amd/libpartls_hip_parent.so"
cd "$TMP/partitionedls.jl_amd/csrc"
$HIPCC $FLAGS -DPARTLS_ONLY_T=16 -c sweep_blk.hip -o "$TMP/sweep_blk_t16.o"
$HIPCC -shared -fPIC --offload-arch=gfx950 -o "$ROOT/partitionedls.jl_amd/libpartls_hip_parent_t16.so" $(ls _build/*.o | grep -v /sweep_blk.o) "$TMP/sweep_blk_t16.o" -ldl
ls -la "$ROOT"/partitionedls.jl_amd/*.so
