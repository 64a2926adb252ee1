"""Build libswarmenv.so (the HIP kernels + C ABI) in-tree for gfx950.

hipcc cross-compiles without a GPU.  -ffp-contract=off is REQUIRED: the kernels reproduce the
reference's IEEE-double operation order (no FMA), see csrc/swarm_env.hip.  The env library is four sources: swarm_env.hip
(the step kernel, by far the longest compile), env_large.hip (the two large-swarm step kernels), env_kernels.hip (the side
kernels) and env_api.hip (the handle and the C ABI).
"""
import os
import shutil
import subprocess

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
SRCS = [os.path.join(PKG, "csrc", f) for f in ("swarm_env.hip", "env_large.hip", "env_kernels.hip", "env_api.hip", "legacy_shim.hip",
                                               "policy_mlp.hip", "rollout.hip", "rule_expert.hip")]
INC = os.path.join(ROOT, "include")
LIB_DIR = os.path.join(PKG, "lib")
LIB = os.path.join(LIB_DIR, "libswarmenv.so")
# what every source is compiled with, here and in tools/isa_diff.py (the include directory and -DSWARM_STAMPS come on top)
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC"]


def hipcc_path():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm's hipcc to build libswarmenv.so)")


def needs_build():
    if not os.path.exists(LIB):
        return True
    headers = [os.path.join(INC, h) for h in ("swarm_env.h", "swarm_policy.h", "swarm_rollout.h")] + [os.path.join(PKG, "csrc", h) for h in ("swarm_internal.h", "env_types.h")]
    newest = max([os.path.getmtime(s) for s in SRCS + headers])
    return os.path.getmtime(LIB) < newest


def build_lib(force=False, verbose=False, stamps=False):
    """stamps=True builds the DIAGNOSTIC library libswarmenv_stamps.so (per-phase in-kernel clocks, used by
    tools/phase_profile.py); its timings are never quoted as product numbers."""
    out = LIB if not stamps else os.path.join(LIB_DIR, "libswarmenv_stamps.so")
    if not stamps and not force and not needs_build():
        return LIB
    os.makedirs(LIB_DIR, exist_ok=True)
    cmd = [hipcc_path()] + HIPCC_FLAGS + ["-shared", "-I" + INC] + (["-DSWARM_STAMPS"] if stamps else []) + SRCS + ["-o", out]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


if __name__ == "__main__":
    print(build_lib(force=True, verbose=True))
