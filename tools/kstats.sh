#!/bin/bash
# Register / scratch / code-size statistics of the k_env instantiations (cross-compiled, no GPU needed).  The headline
# kernel sits at 80 VGPRs (6 waves per SIMD) and ~58 KB of code (64 KB instruction cache): a change that spills or pushes
# the code past the cache costs far more than it saves -- check after every kernel edit.
# The compile commands are marl_llm_amd/build.py's (--cmd UNIT); the six kernel units of the step kernel are compiled side by
# side, as many at a time as the build allows itself.
R=$(cd $(dirname $0)/.. && pwd)
T=$(mktemp -d)
cd $R
CMD() { python3 -m marl_llm_amd.build --cmd $1; }
JOBS=$(python3 -c "from marl_llm_amd.build import jobs; print(jobs())")
# every k_env instantiation is listed, by its template arguments as the symbol spells them: I Li<NPAD>E <f|d|DF16b = OBS_T>
# Lb<DO_STEP>E Lb<LAT>E Lb<HALF>E Lb<FILT>E.  USE_ASM=<file>: read a kept assembly (KEEP_ASM) instead of compiling the step kernel.
S=$T/swarm_env.s
if [ -n "$USE_ASM" ]; then cp $USE_ASM $S; else
for N in 256 128 64 32 16 8; do mkdir $T/n$N; echo "cd $T/n$N && $(CMD swarm_env_n$N) --save-temps -c -o o.o 2>/dev/null"; done | xargs -P $JOBS -d '\n' -n 1 bash -c
cat $T/n*/swarm_env-hip-amdgcn-amd-amdhsa-gfx950.s > $S
fi
cd $T
for SYM in $(grep -o "^_ZN12_GLOBAL__N_15k_envI[A-Za-z0-9_]*:" $S | tr -d : | sort); do
  K=${SYM#_ZN12_GLOBAL__N_15k_env}; K=${K%%EEv*}
  L=$(grep -n "^${SYM}:" $S | cut -d: -f1)
  E=$(awk -v L=$L 'NR>L && /\.end_amdhsa_kernel/{print NR; exit}' $S)
  echo "k_env<$K>" $(awk -v L=$L 'NR>L && /; (NumVgprs|ScratchSize|Occupancy|codeLenInByte)/{printf "%s ", $0; n++} n>=4{exit}' $S) "; spill instructions:" $(sed -n "${L},${E}p" $S | grep -c "Folded Spill\|Folded Reload")
done
# the large-swarm step kernels (env_large: no scratch, no spill in the pair, cell or filter loops), the env's side kernels, the policy kernel (VGPRs must not move: 218 for the bf16 instantiations), its wide geometry (policy_wide: no scratch in any instantiation), the rollout loop's kernels
# and the rule expert (no scratch)
for F in env_large env_kernels policy_mlp policy_wide rollout rule_expert; do
  $(cd $R && CMD $F) -c -o $T/$F.o \
      -Rpass-analysis=kernel-resource-usage 2>&1 | sed -n 's/.*remark: *//p' | sed 's/ \[-Rpass-analysis.*//' |
    awk '/^Function Name:/{if (l) print l; l=$3; next} /^(VGPRs|AGPRs|ScratchSize|Occupancy)/{l=l" ; "$0} END{if (l) print l}'
done
[ -n "$KEEP_ASM" ] && cp $S $KEEP_ASM
rm -rf $T
