"""CPU: tools/asm_diff.py, the comparison that proves a refactor of a kernel file left every kernel's code alone: a kernel whose
local labels were renumbered counts as identical; a changed operand or a changed register count in the descriptor does not."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import asm_diff  # noqa: E402

OLD = """
	.text
	.protected	_Z1kPf
	.globl	_Z1kPf
	.type	_Z1kPf,@function
_Z1kPf:                                 ; @_Z1kPf
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_mov_b32_e32 v1, 0
	s_cbranch_scc1 .LBB3_2
; %bb.1:
	v_add_f32_e32 v1, v1, v0
.LBB3_2:
	s_waitcnt lgkmcnt(0)
	global_store_dword v0, v1, s[0:1]
	s_endpgm
	.section	.rodata,"a",@progbits
	.p2align	6, 0x0
	.amdhsa_kernel _Z1kPf
		.amdhsa_group_segment_fixed_size 0
		.amdhsa_next_free_vgpr 2
		.amdhsa_next_free_sgpr 6
	.end_amdhsa_kernel
	.text
.Lfunc_end3:
	.size	_Z1kPf, .Lfunc_end3-_Z1kPf
"""


def _compare(tmp_path, new_text, renames=()):
    old, new = tmp_path / "old.s", tmp_path / "new.s"
    old.write_text(OLD)
    new.write_text(new_text)
    return asm_diff.compare(str(old), str(new), renames)


def test_labels_operands_descriptor(tmp_path):
    new = OLD.replace(".LBB3_2", ".LBB7_2").replace(".Lfunc_end3", ".Lfunc_end7")
    assert _compare(tmp_path, new) == ([], [], ["_Z1kPf"], [])
    # ... also under a new name, given as a pair; without the pair the kernel is gone and another one is new
    renamed = new.replace("_Z1kPf", "_Z2k2Pf")
    assert _compare(tmp_path, renamed, [("_Z1kPf", "_Z2k2Pf")]) == ([], [], ["_Z1kPf"], [])
    assert _compare(tmp_path, renamed) == (["_Z1kPf"], ["_Z2k2Pf"], [], [])

    assert _compare(tmp_path, OLD.replace("v_add_f32_e32 v1, v1, v0", "v_add_f32_e32 v1, v0, v0")) == ([], [], [], ["_Z1kPf"])
    # a branch to another block is a change too: only the function's number is dropped from a label, not the block's
    assert _compare(tmp_path, OLD.replace("s_cbranch_scc1 .LBB3_2", "s_cbranch_scc1 .LBB3_1")) == ([], [], [], ["_Z1kPf"])

    assert _compare(tmp_path, OLD.replace(".amdhsa_next_free_vgpr 2", ".amdhsa_next_free_vgpr 3")) == ([], [], [], ["_Z1kPf"])
