#!/bin/bash
# usage: tools/valu_lat.sh [build|run <outfile>]
# The VALU latency probe (tools/ubench/valu_lat.hip): `build` compiles it for gfx950 (no GPU
# needed), `run` runs the built program once under a time limit and keeps its output.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
B=$R/tools/ubench/valu_lat
case ${1:-run} in
  build)
    ${HIPCC:-/opt/rocm/bin/hipcc} -O2 -std=c++17 --offload-arch=gfx950 -o $B $B.hip ;;
  run)
    [ -x $B ] || { echo "build it first: tools/valu_lat.sh build"; exit 2; }
    O=${2:-/dev/stdout}
    timeout -k 10 60 $B | tee $O ;;
  *) echo "usage: $0 [build|run <outfile>]"; exit 9 ;;
esac
