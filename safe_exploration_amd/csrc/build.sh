#!/bin/bash
# Builds libsxamd.so (gfx950 code object, host code for this machine) next to the sources.  The translation units are
# compiled in parallel (objects under build/, which is git-ignored) and linked into one shared library.
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OUT=${SX_OUT:-libsxamd.so}
SRCS="sx_runtime.hip sx_gp_fit.hip sx_gp_select.hip sx_gp_predict.hip sx_big.hip sx_gp_rollout.hip sx_feat.hip sx_mlp.hip sx_rank.hip sx_rw_ns1.hip sx_rw_ns2.hip sx_rw_ns3.hip sx_rw_ns4.hip sx_stream_ns12.hip sx_stream_ns34.hip sx_stream_multi.hip sx_stream_starts.hip sx_model_multi.hip sx_perf.hip sx_perf_var.hip sx_perf_multi.hip sx_perf_taylor.hip sx_perf_taylor_multi.hip sx_cautious.hip sx_sat_cost.hip sx_perf_taylor_sat.hip sx_perf_taylor_sat_multi.hip sx_cautious_sat.hip sx_cautious_multi.hip sx_cautious_sat_multi.hip sx_stream_sat.hip sx_stream_sat_multi.hip sx_conset.hip sx_stream_cons.hip sx_stream_cons_sat.hip sx_stream_cons_multi.hip sx_stream_cons_sat_multi.hip sx_stream_starts_cons.hip sx_stream_starts_multi.hip sx_stream_starts_cons_multi.hip sx_gp_append.hip sx_stream_gains.hip sx_gp_drop.hip"
# rebuild only when a source is newer than the library
if [ -f "$OUT" ] && [ -z "$(find . ../../include -newer "$OUT" \( -name '*.hip' -o -name '*.hpp' -o -name '*.h' -o -name 'build.sh' \) | head -1)" ]; then
    exit 0
fi
OBJ=${SX_OBJDIR:-build}
mkdir -p "$OBJ"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -mllvm -amdgpu-mfma-vgpr-form=1 -Wall -Wno-unused-function ${SX_EXTRA_FLAGS:-}"
pids=()
objs=()
for src in $SRCS; do
    obj="$OBJ/${src%.hip}.o"
    objs+=("$obj")
    "$HIPCC" $FLAGS -c "$src" -o "$obj" &
    pids+=($!)
done
for pid in "${pids[@]}"; do wait "$pid"; done
"$HIPCC" --offload-arch=gfx950 -fPIC -shared -o "$OUT.tmp" "${objs[@]}"
mv "$OUT.tmp" "$OUT"
