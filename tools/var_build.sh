#!/bin/bash
# Build a variant of liblsmblk.so with extra -D flags (experiments): tools/var_build.sh NAME -DFOO=1 ...
# -> lsm_amd/var_NAME.so, selected at run time by LSMBLK_SO_OVERRIDE.  The source list is the
# product's (lsm_amd/_build.py: SOURCES).
set -e
cd "$(dirname "$0")/.."
NAME=$1; shift
mapfile -t SRC < <(python3 -c 'import runpy; print("\n".join(runpy.run_path("lsm_amd/_build.py")["SOURCES"]))')
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wall -Wshadow -Wno-unused-function -DLSMBLK_DIAG_BUILD=${DIAG:-0} "$@" -Iinclude \
  "${SRC[@]}" \
  -o lsm_amd/var_$NAME.so
