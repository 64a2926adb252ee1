"""tools/isa_diff.py, same units in both trees: a kernel added to a file renumbers the local labels of the functions the
compiler emits behind it (.LBB<k>_ carries the function's position).  That number is not device code: the kernels behind the
new one still compare identical, and a moved branch target still counts.  Hand-written assembly, nothing is compiled."""
import pytest

from test_isa_diff import A, B, C, HEAD, kernel, tool          # noqa: F401 -- tool is the module-scoped fixture


def test_a_kernel_added_in_front_renumbers_labels_and_nothing_differs(tool):
    branch = kernel("_Z1dv", "\ts_cbranch_scc1 .LBB0_1\n\t.long .Ltmp3-.Lfunc_end0")
    moved = branch.replace(".LBB0_", ".LBB1_").replace(".Ltmp3", ".Ltmp5").replace(".Lfunc_end0", ".Lfunc_end1")
    assert moved != branch
    r = tool.compare(HEAD + A + branch, HEAD + A + C + moved)
    assert r["only_tree"] == ["_Z1cv"] and r["only_base"] == [] and r["differing"] == [] and not r["outside"]


def test_a_moved_branch_target_still_counts(tool):
    branch = kernel("_Z1dv", "\ts_cbranch_scc1 .LBB0_1\n.LBB0_2:")
    r = tool.compare(HEAD + branch, HEAD + C + branch.replace("scc1 .LBB0_1", "scc1 .LBB1_2").replace(".LBB0_2:", ".LBB1_2:").replace(".LBB0_1:", ".LBB1_1:"))
    assert [(d[0], d[2], d[3]) for d in r["differing"]] == [("_Z1dv", "\ts_cbranch_scc1 .LBB_1", "\ts_cbranch_scc1 .LBB_2")]
    # comments and every other line still count in this mode
    r = tool.compare(HEAD + A, HEAD + A.replace("v_add_u32_e32 v1, v0, v0", "v_add_u32_e32 v1, v0, v0 ; note"))
    assert len(r["differing"]) == 1
