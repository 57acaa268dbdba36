#!/bin/bash
# Build the working tree's library with extra compiler flags into build/lib_<NAME>/ for
# A/B runs (scripts/ab_knn_libs.sh):  bash scripts/build_variant.sh w6 -DGF_STEP_WAVES_KNN=6
# The sources are the Makefile's (csrc/sources.mk); the objects go to build/obj_<NAME>.
set -e
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$ROOT/build/lib_$NAME"
make -B -C "$ROOT/gym-flock_amd/csrc" -j"${MAX_JOBS:-8}" OUT="$ROOT/build/lib_$NAME/libgymflock.so" OBJDIR="$ROOT/build/obj_$NAME" \
  CXXFLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wno-unused-result -Wno-unused-value $*"
echo "built build/lib_$NAME ($*)"
