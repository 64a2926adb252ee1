#!/usr/bin/env python3
"""Is the device code of this tree the device code of BASE_REF?  For a refactor that must not move an instruction.

    python3 tools/isa_diff.py BASE_REF [-DNAME[=VALUE] ...] [source ...]

Checks BASE_REF out into a temporary directory, compiles every source (default: the library's, marl_llm_amd.build.SRCS) from
both trees to gfx950 assembly with the library's own flags (marl_llm_amd.build.HIPCC_FLAGS) and compares the text: whole
files first; where two files differ, kernel by kernel -- from `<symbol>:` to `.end_amdhsa_kernel`, so a kernel's register
counts, LDS and scratch sizes (.amdhsa_*) are compared with its instructions.  Prints the kernels that are only in the
base, only in the tree, or different (with the first differing line), then `kernels N, lines M, differing K`, and exits
non-zero if K > 0, the sets of names differ, or two files differ outside their kernels.  Arguments that start with `-` go
to the compiler (-DSWARM_STAMPS, -DSWARM_ONLY_NPAD=64).  No GPU is needed: hipcc cross-compiles.

One name is taken out of both texts before they are compared: `__hip_cuid_<hash>`, a one-byte object that hipcc names after
a hash of the SOURCE text, comments included -- it differs whenever the source does and says nothing about the code."""
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_JOBS = 16


def split_kernels(text):
    """{kernel symbol: its lines, `<symbol>:` .. `.end_amdhsa_kernel`} of one assembly file, and the lines outside them."""
    lines = text.splitlines()
    names = set(m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m)
    kernels, outside, cur = {}, [], None
    for l in lines:
        if cur is None:
            m = re.match(r"([^\s:]+):", l)
            if m and m.group(1) in names:
                cur = kernels.setdefault(m.group(1), [])
        (outside if cur is None else cur).append(l)
        if cur is not None and l.strip() == ".end_amdhsa_kernel":
            cur = None
    return kernels, outside


def strip_cuid(text):
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", text)


def compare(base_text, tree_text):
    """Compare two assembly files.  Returns a dict: kernels (names in either), lines (of tree_text), only_base, only_tree
    (sorted names), differing ([(name, line number inside the kernel from 1, base line, tree line)]; a missing line is
    None), outside (True if the files differ, but in no kernel)."""
    res = {"lines": len(tree_text.splitlines()), "only_base": [], "only_tree": [], "differing": [], "outside": False}
    kb, kt = split_kernels(base_text)[0], split_kernels(tree_text)[0]
    res["kernels"] = len(set(kb) | set(kt))
    if base_text == tree_text:
        return res
    res["only_base"] = sorted(set(kb) - set(kt))
    res["only_tree"] = sorted(set(kt) - set(kb))
    for name in sorted(set(kb) & set(kt)):
        a, b = kb[name], kt[name]
        if a != b:
            n = next((q for q in range(min(len(a), len(b))) if a[q] != b[q]), min(len(a), len(b)))
            res["differing"].append((name, n + 1, a[n] if n < len(a) else None, b[n] if n < len(b) else None))
    res["outside"] = not (res["only_base"] or res["only_tree"] or res["differing"])
    return res


def checkout(ref, dst):
    """the committed files of `ref` under dst (git archive | tar: no worktree to register and prune)"""
    ar = subprocess.Popen(["git", "-C", ROOT, "archive", "--format=tar", ref], stdout=subprocess.PIPE)
    subprocess.check_call(["tar", "-x", "-C", dst], stdin=ar.stdout)
    ar.stdout.close()
    if ar.wait() != 0:
        raise RuntimeError("git archive %s failed" % ref)


def compile_asm(hipcc, flags, root, rel, out):
    """rel (relative to root) -> device assembly `out`; run from the tree's root so that both trees' .file lines agree"""
    if not os.path.exists(os.path.join(root, rel)):
        return None
    cmd = [hipcc] + flags + ["-Iinclude", "--cuda-device-only", "-S", rel, "-o", out]
    p = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if p.returncode != 0:
        raise RuntimeError("%s (in %s) failed:\n%s" % (" ".join(cmd), root, p.stdout))
    with open(out) as f:
        return strip_cuid(f.read())


def main(argv):
    from marl_llm_amd.build import HIPCC_FLAGS, SRCS, hipcc_path
    args = [a for a in argv if not a.startswith("-")]
    extra = [a for a in argv if a.startswith("-")]
    if not args or "-h" in extra or "--help" in extra:
        print(__doc__)
        return 2
    base_ref = args[0]
    rels = [os.path.relpath(os.path.abspath(s), ROOT) for s in args[1:]] or [os.path.relpath(s, ROOT) for s in SRCS]
    hipcc, flags = hipcc_path(), HIPCC_FLAGS + extra
    tmp = tempfile.mkdtemp(prefix="isa_diff_")
    try:
        base_root, out = os.path.join(tmp, "base"), os.path.join(tmp, "out")
        os.makedirs(base_root)
        os.makedirs(out)
        checkout(base_ref, base_root)
        jobs = max(1, min(MAX_JOBS, os.cpu_count() or 1))
        with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
            # the longest compile (the step kernel, first in SRCS) is started first, for both trees
            fut = {(side, rel): pool.submit(compile_asm, hipcc, flags, root, rel,
                                            os.path.join(out, "%s_%d.s" % (side, q)))
                   for q, rel in enumerate(rels) for side, root in (("base", base_root), ("tree", ROOT))}
            asm = {k: f.result() for k, f in fut.items()}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    kernels = lines = differing = 0
    bad = False
    for rel in rels:
        b, t = asm[("base", rel)], asm[("tree", rel)]
        if b is None and t is None:
            print("%s: in neither tree" % rel)
            bad = True
            continue
        r = compare(b or "", t or "")
        kernels += r["kernels"]
        lines += r["lines"]
        differing += len(r["differing"])
        bad = bad or bool(r["only_base"] or r["only_tree"] or r["differing"] or r["outside"])
        print("%s: %s" % (rel, "identical" if b == t else "DIFFERENT"))
        for name in r["only_base"]:
            print("  only in %s: %s" % (base_ref, name))
        for name in r["only_tree"]:
            print("  only in the tree: %s" % name)
        for name, n, lb, lt in r["differing"]:
            print("  differs: %s, first at line %d of the kernel\n    %s: %s\n    tree: %s" % (name, n, base_ref, lb, lt))
        if r["outside"]:
            print("  the text outside the kernels differs")
    print("kernels %d, lines %d, differing %d" % (kernels, lines, differing))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
