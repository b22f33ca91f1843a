#!/bin/bash
# Builds and runs tools/sanitize_koopman_lmpc.hip: a stand-alone program (its own main, no interpreter, CPU only) that drives the host
# side of edmdc_lmpc_step / edmdc_lmpc_step_dev under AddressSanitizer and UndefinedBehaviourSanitizer.  The host code under test
# (capi.hip, which the program includes to make a brov_ctx without a device) is compiled here with the sanitizers; the other
# sources' objects come from the ordinary build (bluerov2_dynamics_amd/_build.py names them).
# Usage: tools/sanitize_koopman_lmpc.sh [build directory]      (default: a fresh temporary directory)
set -eu -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:-$(mktemp -d)}
mkdir -p "$OUT"
OBJS=$(python - <<PY
import os
from bluerov2_dynamics_amd import _build
_build.build_library()
print(" ".join(os.path.join(_build.CSRC, "build", s.replace(".hip", ".o")) for s in _build.SOURCES if s != "capi.hip"))
PY
)
HIPCC=$(command -v hipcc || echo /opt/rocm/bin/hipcc)
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer"
"$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -DBROV2_BUILDING=1 $(for f in $SAN; do printf -- "-Xarch_host %s " "$f"; done) \
    -I bluerov2_dynamics_amd/csrc -c tools/sanitize_koopman_lmpc.hip -o "$OUT/sanitize_koopman_lmpc.o"
"$HIPCC" --offload-arch=gfx950 "$OUT/sanitize_koopman_lmpc.o" $OBJS -fsanitize=address,undefined -ldl -o "$OUT/sanitize_koopman_lmpc"
ASAN_OPTIONS=detect_leaks=0 "$OUT/sanitize_koopman_lmpc"
