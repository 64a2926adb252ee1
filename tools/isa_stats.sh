#!/bin/bash
# static instruction mix of one kernel of the env library -- diagnostics only.  $1: a regular expression for the kernel's
# mangled name (default: k_env<64, float, step, lattice, full geometry, unfiltered>), $2: where to leave the assembly, $3: the
# unit of marl_llm_amd/build.py that holds the kernel (default: swarm_env_n64, the step kernel's unit of 64 agents;
# env_kernels for the side kernels).  Only that unit is compiled, by build.py's own command.
set -e
OUT=${2:-/tmp/swarm_env.s}
$(python3 -m marl_llm_amd.build --cmd ${3:-swarm_env_n64}) -S --cuda-device-only -o "$OUT"
SYM=${1:-_ZN12_GLOBAL__N_15k_envILi64EfLb1ELb1ELb0ELb0EEEv[A-Za-z0-9_]*}
awk -v sym="$SYM" '$0 ~ "^"sym":" {on=1} on && /s_endpgm/ {print; on=0} on {print}' "$OUT" > /tmp/kfn.s
echo "lines: $(wc -l < /tmp/kfn.s)"
echo "VALU: $(grep -cE '^\s+v_' /tmp/kfn.s)  SALU: $(grep -cE '^\s+s_' /tmp/kfn.s)  LDS: $(grep -cE '^\s+ds_' /tmp/kfn.s)  global: $(grep -cE '^\s+global_' /tmp/kfn.s) scratch: $(grep -cE '^\s+scratch_' /tmp/kfn.s)"
grep -E "^\s+\.(vgpr_count|sgpr_count|lds_size)|NumVgprs|NumSgprs|ScratchSize|Occupancy" "$OUT" | head -0
awk -v sym="$SYM" '$0 ~ "\\.name:.*"sym {on=1} on && /(vgpr_count|sgpr_count|private_segment_fixed_size)/ {print} on && /\.wavefront_size/ {on=0}' "$OUT"
