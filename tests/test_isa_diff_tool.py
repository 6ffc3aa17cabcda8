"""tools/isa_diff.py judges "byte-identical": a kernel emitted at another position in the file (the function number inside its local
labels, and the column padding behind such a label, move) is the same kernel; a changed instruction is not."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LISTING = """\
k1:                                     ; @k1
{label}{pad}; =>This Inner Loop Header: Depth=1
\tv_add_f32_e32 v0, v1, v2
\t{insn}
\ts_cbranch_scc1 {target}
\ts_endpgm
.Lfunc_end{n}:
\t.amdhsa_kernel k1
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_private_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr 3
\t\t.amdhsa_next_free_sgpr 8
\t.end_amdhsa_kernel
"""


def listing(tmp_path, name, n, insn="v_mul_f32_e32 v0, v0, v1"):
    label = f".LBB{n}_3:"
    p = tmp_path / name
    p.write_text(LISTING.format(label=label, pad=" " * (40 - len(label)), insn=insn, target=f".LBB{n}_3", n=n))
    return str(p)


def run(a, b):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_diff.py"), a, b], capture_output=True, text=True)
    return out.returncode, out.stdout.strip().splitlines()[-1]


def test_another_function_number_and_its_padding_are_the_same_kernel(tmp_path):
    rc, line = run(listing(tmp_path, "old.s", 9), listing(tmp_path, "new.s", 10))       # one more digit: one column less padding
    assert rc == 0 and "byte-identical 1, registers only renamed 0, other differences 0, unpaired 0" in line, line


def test_a_renamed_register_is_not_byte_identical(tmp_path):
    rc, line = run(listing(tmp_path, "old.s", 9), listing(tmp_path, "new.s", 9, insn="v_mul_f32_e32 v0, v0, v2"))
    assert rc == 0 and "byte-identical 0, registers only renamed 1" in line, line


def test_a_changed_instruction_fails(tmp_path):
    rc, line = run(listing(tmp_path, "old.s", 9), listing(tmp_path, "new.s", 10, insn="v_fma_f32 v0, v0, v1, v2"))
    assert rc == 1 and "byte-identical 0" in line and "other differences 1" in line, line
