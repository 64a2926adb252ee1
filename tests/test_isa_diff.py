"""tools/isa_diff.py's splitter and comparer on hand-written assembly (CPU only, nothing is compiled): two files that are
the same, one kernel changed, one kernel added, the same kernels in another order."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel(name, body, vgprs=8):
    return """\t.globl\t%(n)s
\t.type\t%(n)s,@function
%(n)s:                                  ; @%(n)s
; %%bb.0:
%(b)s
.LBB0_1:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel %(n)s
\t\t.amdhsa_next_free_vgpr %(v)d
\t.end_amdhsa_kernel
\t.text
.Lfunc_end_%(n)s:
\t.size\t%(n)s, .Lfunc_end_%(n)s-%(n)s
""" % {"n": name, "b": body, "v": vgprs}


HEAD = '\t.text\n\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"\n'
A = kernel("_Z1av", "\tv_mov_b32_e32 v0, 0\n\tv_add_u32_e32 v1, v0, v0")
B = kernel("_Z1bv", "\ts_load_dwordx2 s[0:1], s[4:5], 0x0\n\ts_waitcnt lgkmcnt(0)")
B_MOVED = kernel("_Z1bv", "\ts_load_dwordx2 s[0:1], s[4:5], 0x8\n\ts_waitcnt lgkmcnt(0)")
C = kernel("_Z1cv", "\ts_nop 0")


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("isa_diff", os.path.join(ROOT, "tools", "isa_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_split_takes_symbol_to_descriptor_end(tool):
    kernels, outside = tool.split_kernels(HEAD + A + B)
    assert sorted(kernels) == ["_Z1av", "_Z1bv"]
    a = kernels["_Z1av"]
    assert a[0].startswith("_Z1av:") and a[-1].strip() == ".end_amdhsa_kernel"
    assert "\t\t.amdhsa_next_free_vgpr 8" in a and "\tv_add_u32_e32 v1, v0, v0" in a
    assert ".LBB0_1:" in a                                   # a local label does not end a kernel
    assert not any("v_add_u32" in l or ".amdhsa_next_free_vgpr" in l for l in outside)
    assert len(a) + len(kernels["_Z1bv"]) + len(outside) == len((HEAD + A + B).splitlines())


def test_identical(tool):
    r = tool.compare(HEAD + A + B, HEAD + A + B)
    assert r["kernels"] == 2 and r["lines"] == len((HEAD + A + B).splitlines())
    assert r["only_base"] == [] and r["only_tree"] == [] and r["differing"] == [] and not r["outside"]


def test_one_kernel_changed(tool):
    r = tool.compare(HEAD + A + B, HEAD + A + B_MOVED)
    assert r["kernels"] == 2 and r["only_base"] == [] and r["only_tree"] == [] and not r["outside"]
    assert r["differing"] == [("_Z1bv", 3, "\ts_load_dwordx2 s[0:1], s[4:5], 0x0", "\ts_load_dwordx2 s[0:1], s[4:5], 0x8")]
    # a descriptor line counts as much as an instruction
    r = tool.compare(HEAD + A + B, HEAD + kernel("_Z1av", "\tv_mov_b32_e32 v0, 0\n\tv_add_u32_e32 v1, v0, v0", vgprs=9) + B)
    assert [(d[0], d[2], d[3]) for d in r["differing"]] == [("_Z1av", "\t\t.amdhsa_next_free_vgpr 8", "\t\t.amdhsa_next_free_vgpr 9")]


def test_one_kernel_added(tool):
    r = tool.compare(HEAD + A + B, HEAD + A + B + C)
    assert r["kernels"] == 3 and r["only_tree"] == ["_Z1cv"] and r["only_base"] == [] and r["differing"] == []
    r = tool.compare(HEAD + A + B + C, HEAD + A + B)
    assert r["only_base"] == ["_Z1cv"] and r["only_tree"] == [] and r["differing"] == []


def test_difference_outside_the_kernels_is_reported(tool):
    r = tool.compare(HEAD + A, HEAD + A + '\t.ident\t"other compiler"\n')
    assert r["differing"] == [] and r["only_base"] == [] and r["only_tree"] == [] and r["outside"]


def test_kernels_in_another_order_are_reordered_not_outside(tool):
    r = tool.compare(HEAD + A + B, HEAD + B + A)
    assert r["kernels"] == 2 and r["differing"] == [] and r["only_base"] == [] and r["only_tree"] == []
    assert r["reordered"] and not r["outside"]
    # the function number of a label outside the kernels moves with the order and does not count
    r = tool.compare(HEAD + A + ".Lfunc_end0:\n" + B + ".Lfunc_end1:\n", HEAD + B + ".Lfunc_end0:\n" + A + ".Lfunc_end1:\n")
    assert r["reordered"] and not r["outside"] and r["differing"] == []
    # the same file is neither
    r = tool.compare(HEAD + A + B, HEAD + A + B)
    assert not r["reordered"] and not r["outside"]


def test_another_order_and_another_line_outside_is_outside(tool):
    r = tool.compare(HEAD + A + B, HEAD + B + A + '\t.ident\t"other compiler"\n')
    assert r["differing"] == [] and r["only_base"] == [] and r["only_tree"] == []
    assert r["outside"] and not r["reordered"]
    # a line that is there twice is not the line once: multisets, not sets
    r = tool.compare(HEAD + A + B, HEAD + B + A + '\t.text\n')
    assert r["outside"] and not r["reordered"]
    # a changed kernel in another order is a changed kernel
    r = tool.compare(HEAD + A + B, HEAD + B_MOVED + A)
    assert [d[0] for d in r["differing"]] == ["_Z1bv"] and not r["reordered"] and not r["outside"]


# ---- one source cut into different units in the two trees: kernel by kernel over all units, local labels and comments normalised

def metadata(entries):
    return "\t.amdgpu_metadata\n---\namdhsa.kernels:\n" + "".join(
        "  - .args:\n      - .name:           P\n        .size:           %d\n    .name:           %s\n    .symbol:         %s.kd\n"
        % (size, n, n) for n, size in entries) + "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n\n\t.end_amdgpu_metadata\n"


def test_units_function_number_and_comments_do_not_count(tool):
    # the same kernel as the first function of a unit and as the eighth of the whole file
    whole = HEAD + B + A + metadata([("_Z1bv", 8), ("_Z1av", 8)])
    a_unit = HEAD + A.replace(".LBB0_1", ".LBB7_1").replace("; @_Z1av", "; -- Begin function _Z1av").replace("; %bb.0:", "") + metadata([("_Z1av", 8)])
    b_unit = HEAD + B + metadata([("_Z1bv", 8)])
    assert ".LBB7_1:" in a_unit and "; @_Z1av" not in a_unit
    r = tool.compare_units([whole], [a_unit, b_unit])
    assert r["kernels"] == 2 and r["differing"] == [] and r["only_base"] == [] and r["only_tree"] == [] and r["duplicates"] == []
    assert r["lines"] == len(a_unit.splitlines()) + len(b_unit.splitlines())
    assert tool.normalise(["\ts_cbranch_scc1 .LBB12_3 ; taken", ".LJTI4_0:", "\t.long .Ltmp9-.Lfunc_end33", "; only a comment"]) == \
        ["\ts_cbranch_scc1 .LBB_3", ".LJTI_0:", "\t.long .Ltmp-.Lfunc_end"]


def test_units_branch_target_counts(tool):
    r = tool.compare_units([HEAD + A], [HEAD + A.replace(".LBB0_1", ".LBB0_2")])
    assert [(d[0], d[2], d[3]) for d in r["differing"]] == [("_Z1av", ".LBB_1:", ".LBB_2:")]
    branch = kernel("_Z1dv", "\ts_cbranch_scc1 .LBB0_1\n.LBB0_2:")
    r = tool.compare_units([HEAD + branch], [HEAD + branch.replace("scc1 .LBB0_1", "scc1 .LBB0_2")])
    assert [(d[0], d[2], d[3]) for d in r["differing"]] == [("_Z1dv", "\ts_cbranch_scc1 .LBB_1", "\ts_cbranch_scc1 .LBB_2")]


def test_units_descriptor_and_metadata_count(tool):
    r = tool.compare_units([HEAD + A + B], [HEAD + B, HEAD + kernel("_Z1av", "\tv_mov_b32_e32 v0, 0\n\tv_add_u32_e32 v1, v0, v0", vgprs=9)])
    assert [(d[0], d[2], d[3]) for d in r["differing"]] == [("_Z1av", "\t\t.amdhsa_next_free_vgpr 8", "\t\t.amdhsa_next_free_vgpr 9")]
    r = tool.compare_units([HEAD + A + B + metadata([("_Z1av", 8), ("_Z1bv", 8)])], [HEAD + A + metadata([("_Z1av", 8)]), HEAD + B + metadata([("_Z1bv", 16)])])
    assert [(d[0], d[2], d[3]) for d in r["differing"]] == [("_Z1bv", "        .size:           8", "        .size:           16")]


def test_units_duplicate_kernel_is_reported(tool):
    r = tool.compare_units([HEAD + A + B], [HEAD + A + B, HEAD + A])
    assert r["duplicates"] == [("tree", "_Z1av")] and r["differing"] == [] and r["only_base"] == [] and r["only_tree"] == []
    r = tool.compare_units([HEAD + A, HEAD + A + B], [HEAD + A + B])
    assert r["duplicates"] == [("base", "_Z1av")]
