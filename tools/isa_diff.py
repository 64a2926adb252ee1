#!/usr/bin/env python3
"""Is the device code of this tree the device code of BASE_REF?  For a refactor that must not move an instruction.

    python3 tools/isa_diff.py BASE_REF [-DNAME[=VALUE] ...] [source ...]

Checks BASE_REF out into a temporary directory and compiles, for each tree, the units that tree's own marl_llm_amd/build.py
lists (UNITS; a base without it: its SRCS, one unit each) to gfx950 assembly with that file's flags (HIPCC_FLAGS), all in
parallel, and compares the text source by source (default: every source of the library).

Where both trees compile a source as the same unit(s), unit by unit: whole files first; where two files differ, kernel by kernel -- from
`<symbol>:` to `.end_amdhsa_kernel`, so a kernel's register counts, LDS and scratch sizes (.amdhsa_*) are compared with its
instructions.  One name is taken out of both texts before they are compared: `__hip_cuid_<hash>`, a one-byte object that
hipcc names after a hash of the SOURCE text, comments included -- it differs whenever the source does and says nothing about
the code.  Kernel by kernel, the number that the local labels .LBB<k>_, .Lfunc_end<k>, .LJTI<k>_ and .Ltmp<k> carry is taken
out as well: it is the function's position in its translation unit, and a kernel added to a file moves it for every function
the compiler emits behind the new one (template instantiations come last) without touching an instruction.  Two files whose
kernels are all the same but come out in another order are not a changed file: the lines outside the kernels are then
compared as multisets, after the same treatment of the labels, and where those are equal the file is reported as reordered.

Where the trees cut a source into different units, the kernels of all of the source's units are compared one by one, each with
its entry of the `amdhsa.kernels` metadata (arguments, segment sizes); a kernel found in two units of one tree is an error,
and the text outside the kernels is not compared.  Two things are taken out of a kernel's text first (normalise): the number
that the local labels .LBB<k>_, .Lfunc_end<k>, .LJTI<k>_ and .Ltmp<k> carry -- the function's position in its translation
unit -- and the `;` comments.  Nothing else.

Prints the kernels that are only in the base, only in the tree, or different (with the first differing line), then
`kernels N, lines M, differing K`, and exits non-zero if K > 0, the sets of names differ, a kernel is there twice, or two
files differ outside their kernels in more than the order of their lines.  Arguments that start with `-` go to the compiler, for every unit (-DSWARM_STAMPS).  No
GPU is needed: hipcc cross-compiles."""
import concurrent.futures
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def unnumbered(lines):
    """a kernel's lines without the number its local labels .LBB<k>_, .LJTI<k>_, .Lfunc_end<k> and .Ltmp<k> carry: the function's
    position in its translation unit, which a kernel added in front of it moves -- and nothing else of its text"""
    out = []
    for l in lines:
        l = re.sub(r"\.(LBB|LJTI)\d+_", r".\1_", l)
        l = re.sub(r"\.(Lfunc_end|Ltmp)\d+", r".\1", l)
        if ";" in l:                                # a comment names blocks as BB<k>_ and is aligned behind the (shorter) label
            code, _, note = l.partition(";")
            l = code.rstrip() + " ;" + re.sub(r"\bBB\d+_", "BB_", note)
        out.append(l)
    return out


def by_name(kb, kt, res):
    """fill res with the names only in kb, only in kt, and the first differing line of those in both"""
    res["only_base"] = sorted(set(kb) - set(kt))
    res["only_tree"] = sorted(set(kt) - set(kb))
    for name in sorted(set(kb) & set(kt)):
        a, b = kb[name], kt[name]
        if a != b:
            n = next((q for q in range(min(len(a), len(b))) if a[q] != b[q]), min(len(a), len(b)))
            res["differing"].append((name, n + 1, a[n] if n < len(a) else None, b[n] if n < len(b) else None))


def compare(base_text, tree_text):
    """Compare two assembly files.  Returns a dict: kernels (names in either), lines (of tree_text), only_base, only_tree
    (sorted names), differing ([(name, line number inside the kernel from 1, base line, tree line)]; a missing line is
    None), reordered (True if the files differ only in the order of their kernels: the same kernels, and outside them the same
    lines as multisets), outside (True if the files differ in no kernel and in more than that order)."""
    res = {"lines": len(tree_text.splitlines()), "only_base": [], "only_tree": [], "differing": [], "outside": False,
           "reordered": False}
    (kb, ob), (kt, ot) = split_kernels(base_text), split_kernels(tree_text)
    res["kernels"] = len(set(kb) | set(kt))
    if base_text == tree_text:
        return res
    by_name({n: unnumbered(k) for n, k in kb.items()}, {n: unnumbered(k) for n, k in kt.items()}, res)
    if not (res["only_base"] or res["only_tree"] or res["differing"]):
        res["reordered"] = sorted(unnumbered(ob)) == sorted(unnumbered(ot))
        res["outside"] = not res["reordered"]
    return res


def normalise(lines):
    """a kernel's lines without the function number of its local labels and without `;` comments (lines that held only a
    comment go)"""
    return [l for l in unnumbered(re.sub(r"\s*;.*$", "", l) for l in lines) if l.strip()]


def kernel_metadata(text):
    """{kernel symbol: the lines of its entry under `amdhsa.kernels:` in the file's metadata}"""
    lines = text.splitlines()
    entries, cur = {}, None
    try:
        q = lines.index("amdhsa.kernels:") + 1
    except ValueError:
        return entries
    while q < len(lines) and (lines[q].startswith("  ") or not lines[q].strip()):
        if lines[q].startswith("  - "):
            cur = []
        if cur is not None:
            cur.append(lines[q])
            m = re.match(r"    \.name:\s+(\S+)", lines[q])
            if m:
                entries[m.group(1)] = cur
        q += 1
    return entries


def compare_units(base_texts, tree_texts):
    """Compare one source's kernels over all of its units in each tree (lists of assembly files).  compare()'s dict, with
    `duplicates`: [(which tree, name)] of kernels that two units of one tree hold; `outside` is False, not compared."""
    res = {"lines": sum(len(t.splitlines()) for t in tree_texts), "only_base": [], "only_tree": [], "differing": [],
           "outside": False, "duplicates": []}
    sides = {}
    for side, texts in (("base", base_texts), ("tree", tree_texts)):
        ks = sides[side] = {}
        for t in texts:
            meta = kernel_metadata(t)
            for name, body in split_kernels(t)[0].items():
                if name in ks:
                    res["duplicates"].append((side, name))
                ks[name] = normalise(body) + meta.get(name, [])
    kb, kt = sides["base"], sides["tree"]
    res["kernels"] = len(set(kb) | set(kt))
    by_name(kb, kt, res)
    return res


def checkout(ref, dst):
    """the committed files of `ref` under dst (git archive | tar: no worktree to register and prune)"""
    ar = subprocess.Popen(["git", "-C", ROOT, "archive", "--format=tar", ref], stdout=subprocess.PIPE)
    subprocess.check_call(["tar", "-x", "-C", dst], stdin=ar.stdout)
    ar.stdout.close()
    if ar.wait() != 0:
        raise RuntimeError("git archive %s failed" % ref)


def tree_units(root):
    """(HIPCC_FLAGS, {source relative to root: [(unit name, its defines)]}) as root's own marl_llm_amd/build.py has them"""
    spec = importlib.util.spec_from_file_location("build_of_" + re.sub(r"\W", "_", root), os.path.join(root, "marl_llm_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    units = {}
    if hasattr(mod, "UNITS"):
        for name, src, defines in mod.UNITS:
            units.setdefault(os.path.join("marl_llm_amd", "csrc", src), []).append((name, list(defines)))
    else:
        for src in mod.SRCS:
            units[os.path.relpath(src, root)] = [(os.path.splitext(os.path.basename(src))[0], [])]
    return mod.HIPCC_FLAGS, units


def compile_asm(hipcc, flags, root, rel, out):
    """rel (relative to root) -> device assembly `out`; run from the tree's root so that both trees' .file lines agree"""
    cmd = [hipcc] + flags + ["-Iinclude", "--cuda-device-only", "-S", rel, "-o", out]
    p = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if p.returncode != 0:
        raise RuntimeError("%s (in %s) failed:\n%s" % (" ".join(cmd), root, p.stdout))
    with open(out) as f:
        return strip_cuid(f.read())


def bad_in(r):
    """does a source's summed result fail the run?"""
    return bool(r["only_base"] or r["only_tree"] or r["differing"] or r["outside"] or r.get("duplicates"))


def main(argv):
    from marl_llm_amd.build import hipcc_path, jobs
    args = [a for a in argv if not a.startswith("-")]
    extra = [a for a in argv if a.startswith("-")]
    if not args or "-h" in extra or "--help" in extra:
        print(__doc__)
        return 2
    base_ref = args[0]
    hipcc = hipcc_path()
    tmp = tempfile.mkdtemp(prefix="isa_diff_")
    try:
        base_root, out = os.path.join(tmp, "base"), os.path.join(tmp, "out")
        os.makedirs(base_root)
        os.makedirs(out)
        checkout(base_ref, base_root)
        trees = {"base": (base_root,) + tree_units(base_root), "tree": (ROOT,) + tree_units(ROOT)}
        rels = [os.path.relpath(os.path.abspath(s), ROOT) for s in args[1:]] or list(trees["tree"][2])
        with concurrent.futures.ThreadPoolExecutor(jobs()) as pool:
            # (both build.py list the longest compiles first)
            fut = {(side, rel): [pool.submit(compile_asm, hipcc, flags + extra + defines, root, rel,
                                             os.path.join(out, "%s_%s.s" % (side, name)))
                                 for name, defines in units.get(rel, [])]
                   for rel in rels for side, (root, flags, units) in trees.items()}
            asm = {k: [f.result() for f in fs] for k, fs in fut.items()}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    kernels = lines = differing = 0
    bad = False
    for rel in rels:
        b, t = asm[("base", rel)], asm[("tree", rel)]
        if not b and not t:
            print("%s: in neither tree" % rel)
            bad = True
            continue
        cut_b, cut_t = ([d for _, d in trees[side][2].get(rel, [])] for side in ("base", "tree"))
        if cut_b == cut_t or not b or not t:
            # the same units in both trees (or a source that one tree lacks): unit by unit, whole files first
            rs = [compare(x, y) for x, y in zip(b, t)] if cut_b == cut_t else [compare(x, "") for x in b] + [compare("", y) for y in t]
            r = {k: sum((q[k] for q in rs), type(rs[0][k])()) for k in rs[0]}
            print("%s: %s" % (rel, "identical" if b == t else "kernels identical, emitted in another order"
                              if r["reordered"] and not bad_in(r) else "DIFFERENT"))
        else:
            r = compare_units(b, t)
            same = not (r["only_base"] or r["only_tree"] or r["differing"] or r["duplicates"])
            print("%s: %d unit(s) in %s, %d in the tree: kernels %s; the text outside the kernels was not compared"
                  % (rel, len(b), base_ref, len(t), "identical" if same else "DIFFERENT"))
        kernels += r["kernels"]
        lines += r["lines"]
        differing += len(r["differing"])
        bad = bad or bad_in(r)
        for side, name in r.get("duplicates", []):
            print("  in two units of %s: %s" % (base_ref if side == "base" else "the tree", name))
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
