#!/bin/bash
# static instruction mix of one kernel of the env library -- diagnostics only.  $1: a regular expression for the kernel's
# mangled name (default: k_env<64, float, step, lattice>), $2: where to leave the assembly, $3: the source
# (swarm_env for k_env, env_kernels for the side kernels)
set -e
OUT=${2:-/tmp/swarm_env.s}
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iinclude -S --cuda-device-only -o "$OUT" marl_llm_amd/csrc/${3:-swarm_env}.hip
SYM=${1:-_ZN12_GLOBAL__N_15k_envILi64EfLb1ELb1ELb0EEEv[A-Za-z0-9_]*}
awk -v sym="$SYM" '$0 ~ "^"sym":" {on=1} on && /s_endpgm/ {print; on=0} on {print}' "$OUT" > /tmp/kfn.s
echo "lines: $(wc -l < /tmp/kfn.s)"
echo "VALU: $(grep -cE '^\s+v_' /tmp/kfn.s)  SALU: $(grep -cE '^\s+s_' /tmp/kfn.s)  LDS: $(grep -cE '^\s+ds_' /tmp/kfn.s)  global: $(grep -cE '^\s+global_' /tmp/kfn.s) scratch: $(grep -cE '^\s+scratch_' /tmp/kfn.s)"
grep -E "^\s+\.(vgpr_count|sgpr_count|lds_size)|NumVgprs|NumSgprs|ScratchSize|Occupancy" "$OUT" | head -0
awk -v sym="$SYM" '$0 ~ "\\.name:.*"sym {on=1} on && /(vgpr_count|sgpr_count|private_segment_fixed_size)/ {print} on && /\.wavefront_size/ {on=0}' "$OUT"
