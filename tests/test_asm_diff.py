"""tools/asm_diff.py on two tiny hand-written folders of assembly (its folders-of-assembly input; no compiler, no GPU): kernels
are paired across the whole library, so one that moved to another file is compared with its former self; one changed
instruction is `differs`; a kernel that one side lacks is listed as such; a template kernel two units instantiate is
compared copy by copy."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "asm_diff.py")

# one kernel as hipcc -S lays it out: label, instructions, kernel descriptor, end label, resource comments
KERNEL = """\t.protected\t{sym}
\t.globl\t{sym}
\t.type\t{sym},@function
{sym}:                                  ; @{sym}
; %bb.0:
{body}\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {sym}
\t\t.amdhsa_group_segment_fixed_size {lds}
\t\t.amdhsa_private_segment_fixed_size 0
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{n}:
\t.size\t{sym}, .Lfunc_end{n}-{sym}
; TotalNumSgprs: {sgpr}
; NumVgprs: {vgpr}
"""
META = """  - .agpr_count:     0
    .name:           {sym}
    .sgpr_spill_count: 0
    .vgpr_spill_count: 0
"""
ADD = "\ts_load_dwordx2 s[0:1], s[4:5], 0x0\n\tv_add_u32_e32 v1, v0, v0\n\ts_cbranch_execz .LBB{n}_2\n.LBB{n}_2:\n"
SUB = ADD.replace("v_add_u32_e32", "v_sub_u32_e32")          # the one instruction that changed
SYM = {"k_stay": "_ZN2hj6k_stayEPj", "k_move": "_ZN2hj6k_moveEPj", "k_edit": "_ZN2hj6k_editEPj", "k_gone": "_ZN2hj6k_goneEPj",
       "k_new": "_ZN2hj5k_newEPj", "k_twice<1>": "_ZN2hj7k_twiceILi1EEEvPj"}


def write_unit(folder, unit, kernels):
    """kernels: [(name, body)]; the local labels carry the kernel's number in the unit, as the compiler's do"""
    text = "\t.text\n" + "".join(KERNEL.format(sym=SYM[k], body=body.format(n=n), n=n, lds=64, sgpr=10, vgpr=2)
                                 for n, (k, body) in enumerate(kernels))
    text += "\t.amdgpu_metadata\n---\namdhsa.kernels:\n" + "".join(META.format(sym=SYM[k]) for k, _ in kernels) + "...\n"
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, unit + ".s"), "w") as f:
        f.write(text)


def run(parent, change):
    out = subprocess.run([sys.executable, TOOL, str(parent), str(change)], capture_output=True, text=True, check=True).stdout
    rows = {}
    for line in out.splitlines():
        cells = [c.strip() for c in line.split("|")]
        if len(cells) >= 4 and cells[2].startswith("`"):
            rows[(cells[1], cells[2].strip("`"))] = cells[3]
    return rows, out.strip().splitlines()[-1]


def test_moved_changed_and_one_sided_kernels(tmp_path):
    parent, change = tmp_path / "parent", tmp_path / "change"
    # the parent has one unit; in the change k_move sits in a new unit, behind another kernel (so its labels are renumbered)
    write_unit(parent, "hj_a", [("k_stay", ADD), ("k_move", ADD), ("k_edit", ADD), ("k_gone", ADD)])
    write_unit(change, "hj_a", [("k_stay", ADD), ("k_edit", SUB)])
    write_unit(change, "hj_b", [("k_new", ADD), ("k_move", ADD)])
    rows, totals = run(parent, change)
    assert rows[("hj_a", "k_stay")] == "identical"
    assert rows[("hj_b", "k_move")] == "identical (parent: hj_a)"
    assert rows[("hj_a", "k_edit")] == "differs"
    assert rows[("hj_a", "k_gone")] == "only in parent"
    assert rows[("hj_b", "k_new")] == "only in change"
    assert len(rows) == 5
    assert totals == "2 kernels identical, 1 differ"


def test_every_copy_of_a_template_kernel_is_compared(tmp_path):
    parent, change = tmp_path / "parent", tmp_path / "change"
    write_unit(parent, "hj_a", [("k_twice<1>", ADD)])
    write_unit(change, "hj_a", [("k_twice<1>", ADD)])
    write_unit(change, "hj_b", [("k_stay", ADD), ("k_twice<1>", SUB)])         # the second object's copy came out differently
    rows, totals = run(parent, change)
    assert rows[("hj_a", "k_twice<1>")] == "identical"
    assert rows[("hj_b", "k_twice<1>")] == "differs (parent: hj_a)"
    assert rows[("hj_b", "k_stay")] == "only in change"
    assert totals == "1 kernels identical, 1 differ"
