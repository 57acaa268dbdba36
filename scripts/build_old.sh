#!/bin/bash
# Build the library of a git revision (default HEAD) into build/lib_old for scripts/ab_libs.sh,
# with that revision's own Makefile (and so its own list of sources).
set -e
REV=${1:-HEAD}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
TMP=$(mktemp -d)
git -C "$ROOT" archive "$REV" gym-flock_amd/csrc include | tar -x -C "$TMP"
mkdir -p "$ROOT/build/lib_old"
make -C "$TMP/gym-flock_amd/csrc" -j"${MAX_JOBS:-8}" OUT="$ROOT/build/lib_old/libgymflock.so"
rm -rf "$TMP"
echo "built build/lib_old from $REV"
