"""Build libswarmenv.so (the HIP kernels + C ABI) in-tree for gfx950.

hipcc cross-compiles without a GPU.  -ffp-contract=off is REQUIRED: the kernels reproduce the
reference's IEEE-double operation order (no FMA), see csrc/swarm_env.hip.

The library is compiled by UNIT (UNITS below), in parallel, each into an object of its own, and linked once.  Almost all of the
compile time is the step kernel, csrc/swarm_env.hip: its 162 instantiations are cut into six units, one per padded agent
count (-DSWARM_ENV_UNIT=<NPAD>), beside a seventh that holds the file's host part (-DSWARM_ENV_UNIT=0); every other source is
one unit.  A unit is compiled again only when its object is missing or older than its source, a header or this file, or when
its command line changed (stale_units), so an edit to env_api.hip costs seconds.  profiles/r13/build_times.txt has the times.

    python -m marl_llm_amd.build               build everything again, verbosely
    python -m marl_llm_amd.build --cmd UNIT    print UNIT's compile command (without -c -o OBJECT): tools/kstats.sh and
                                               tools/isa_stats.sh take the flags from here
"""
import concurrent.futures
import glob
import os
import re
import shlex
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
INC = os.path.join(ROOT, "include")
LIB_DIR = os.path.join(PKG, "lib")
LIB = os.path.join(LIB_DIR, "libswarmenv.so")
# what every unit is compiled with, here and in tools/isa_diff.py (the include directory and the defines come on top)
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC"]
# what is compiled: (unit name, source in csrc/, the unit's own defines), the longest compile first -- the order in which
# build_lib starts them.  swarm_env.hip seven times: its kernels by agent count, then its host part (see that file's head).
UNITS = [("swarm_env_n%d" % n, "swarm_env.hip", ["-DSWARM_ENV_UNIT=%d" % n]) for n in (256, 16, 32, 64, 128, 8)] + [
    ("policy_mlp", "policy_mlp.hip", []),
    ("policy_wide", "policy_wide.hip", []),
    ("rule_expert", "rule_expert.hip", []),
    ("env_large", "env_large.hip", []),
    ("env_kernels", "env_kernels.hip", []),
    ("env_api", "env_api.hip", []),
    ("legacy_shim", "legacy_shim.hip", []),
    ("swarm_env_host", "swarm_env.hip", ["-DSWARM_ENV_UNIT=0"]),
    ("rollout", "rollout.hip", []),
]
MAX_JOBS = 16


def hipcc_path():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm's hipcc to build libswarmenv.so)")


def jobs():
    """compiles at a time: never the machine's CPU count alone (a shared machine shows many more CPUs than a job may use)"""
    cap = [MAX_JOBS, os.cpu_count() or 1]
    if os.environ.get("MAX_JOBS", "").isdigit():
        cap.append(int(os.environ["MAX_JOBS"]))
    return max(1, min(cap))


def all_defines(defines=(), stamps=False):
    return (["-DSWARM_STAMPS"] if stamps else []) + list(defines)


def variant(defines=(), stamps=False):
    """(object directory, library) of a build with these extra defines: every set has its own pair"""
    tag = "".join("_" + re.sub(r"[^\w=.]", "", d[2:]) for d in defines)
    tag = ("_stamps" if stamps else "") + tag
    return os.path.join(LIB_DIR, "obj" + tag), os.path.join(LIB_DIR, "libswarmenv%s.so" % tag)


def unit_cmd(name, defines=(), stamps=False):
    """the compile command of one unit, without `-c -o OBJECT`"""
    src, own = next((s, d) for n, s, d in UNITS if n == name)
    return [hipcc_path()] + HIPCC_FLAGS + ["-I" + INC] + all_defines(defines, stamps) + own + [os.path.join(CSRC, src)]


def stale_units(defines=(), stamps=False):
    """names of the units build_lib would compile: object missing, older than its source, any header or this file, or
    compiled by another command line (kept as text beside the object)"""
    obj_dir = variant(defines, stamps)[0]
    common = glob.glob(os.path.join(INC, "*")) + glob.glob(os.path.join(CSRC, "*.h")) + [os.path.abspath(__file__)]
    newest_common = max(os.path.getmtime(f) for f in common)
    stale = []
    for name, src, _ in UNITS:
        obj = os.path.join(obj_dir, name + ".o")
        try:
            with open(obj + ".cmd") as f:
                same_cmd = f.read() == shlex.join(unit_cmd(name, defines, stamps))
            fresh = same_cmd and os.path.getmtime(obj) >= max(newest_common, os.path.getmtime(os.path.join(CSRC, src)))
        except OSError:
            fresh = False
        if not fresh:
            stale.append(name)
    return stale


def compile_unit(name, obj, cmd, verbose):
    if os.path.exists(obj + ".cmd"):
        os.remove(obj + ".cmd")                     # an interrupted compile leaves no object that counts
    full = cmd + ["-c", "-o", obj]
    if verbose:
        print(shlex.join(full), flush=True)
    p = subprocess.run(full, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if p.returncode != 0:
        raise RuntimeError("compiling %s failed:\n%s\n%s" % (name, shlex.join(full), p.stdout))
    with open(obj + ".cmd", "w") as f:
        f.write(shlex.join(cmd))


def build_lib(force=False, verbose=False, stamps=False, defines=()):
    """Compile the stale units (force: all of them) and link the library; returns its path.  `defines` (["-DNAME=VALUE", ...])
    go to every unit and give the build its own objects and its own library name (SWARM_WPS*, SWARM_EXTRA_SMEM experiments).
    stamps=True is that with -DSWARM_STAMPS: the DIAGNOSTIC library libswarmenv_stamps.so (per-phase in-kernel clocks, used
    by tools/phase_profile.py); its timings are never quoted as product numbers."""
    obj_dir, out = variant(defines, stamps)
    todo = [n for n, _, _ in UNITS] if force else stale_units(defines, stamps)
    objs = [os.path.join(obj_dir, n + ".o") for n, _, _ in UNITS]
    if not todo and os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(o) for o in objs):
        return out
    os.makedirs(obj_dir, exist_ok=True)
    if verbose:
        print("compiling %d of %d units, %d at a time: %s" % (len(todo), len(UNITS), jobs(), " ".join(todo)), flush=True)
    with concurrent.futures.ThreadPoolExecutor(jobs()) as pool:
        futs = [pool.submit(compile_unit, n, os.path.join(obj_dir, n + ".o"), unit_cmd(n, defines, stamps), verbose)
                for n, _, _ in UNITS if n in todo]                            # (UNITS is ordered longest first)
        for f in futs:
            f.result()
    # link beside the library and move the result over it: a failed build leaves the previous library in place
    tmp = "%s.tmp%d" % (out, os.getpid())
    link = [hipcc_path()] + HIPCC_FLAGS + ["-shared"] + objs + ["-o", tmp]
    if verbose:
        print(shlex.join(link), flush=True)
    try:
        subprocess.check_call(link)
        os.replace(tmp, out)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return out


if __name__ == "__main__":
    if sys.argv[1:2] == ["--cmd"]:
        print(shlex.join(unit_cmd(sys.argv[2], sys.argv[3:])))
    else:
        print(build_lib(force=True, verbose=True))
