"""scripts/kernel_streams.py: the splitter, the normaliser and the report on
small hand-written assembly texts (no compiler, no GPU)."""
import importlib.util
import io
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location(
    "kernel_streams", os.path.join(ROOT, "scripts", "kernel_streams.py"))
ks = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ks)

HEAD = """\t.text
\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"
"""


def func(name, label_no, operand="v1", comment="first build"):
    return f"""\t.section\t.text.{name},"axG",@progbits,{name},comdat
\t.globl\t{name} ; -- Begin function {name}
\t.p2align\t8
\t.type\t{name},@function
{name}: ; @{name}
; %bb.0: ; {comment}
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_cmp_gt_i32_e32 vcc, 1, v0
\ts_cbranch_vccnz .LBB{label_no}_2
; %bb.1:
\tv_add_u32_e32 v0, v0, {operand}   ; {comment}
.LBB{label_no}_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr 2
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{label_no}:
\t.size\t{name}, .Lfunc_end{label_no}-{name}
; NumVgprs: 2
"""


TAIL = """\t.amdgpu_metadata
---
amdhsa.kernels:
  - .name: k_same
...
\t.end_amdgpu_metadata
"""

REMARKS = """x.hip:1:1: remark: Function Name: k_same [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark:     TotalSGPRs: 10 [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark:     VGPRs: 2 [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]
x.hip:1:1: remark:     LDS Size [bytes/block]: 0 [-Rpass-analysis=kernel-resource-usage]
"""

BASE = HEAD + func("k_same", 0) + func("k_diff", 1) + func("k_gone", 2) + TAIL
NEW = HEAD + func("k_same", 7, comment="second build") + func("k_diff", 3, operand="v2") + TAIL


def report(must_match=None):
    out = io.StringIO()
    bad = ks.compare(ks.split_kernels(BASE), ks.split_kernels(NEW), ks.parse_remarks(REMARKS),
                     ks.parse_remarks(REMARKS), must_match, out)
    return bad, out.getvalue()


def test_split_keeps_instructions_only():
    k = ks.split_kernels(BASE)
    assert sorted(k) == ["k_diff", "k_gone", "k_same"]       # no metadata key, no data
    assert k["k_same"] == ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "v_cmp_gt_i32_e32 vcc, 1, v0",
                           "s_cbranch_vccnz .L0", "v_add_u32_e32 v0, v0, v1", ".L0:",
                           "s_endpgm"]


def test_labels_and_comments_aside_is_same():
    bad, text = report()
    assert bad == 0
    assert "k_same: same" in text
    assert "vgpr=2 sgpr=10 scratch=0 lds=0 occ=8" in text


def test_changed_operand_differs():
    _, text = report()
    assert "k_diff: differs (6 -> 6 instructions)" in text


def test_symbol_on_one_side_is_missing():
    _, text = report()
    assert "k_gone: missing in new" in text


def test_changed_resources_differ():
    out = io.StringIO()
    k = ks.split_kernels(BASE)
    ks.compare(k, k, ks.parse_remarks(REMARKS),
               ks.parse_remarks(REMARKS.replace("VGPRs: 2", "VGPRs: 3")), None, out)
    assert "k_same: differs" in out.getvalue()


def test_must_match():
    assert report("k_same")[0] == 0
    assert report("k_diff")[0] == 1
    assert report("k_gone")[0] == 1
    assert report("k_")[0] == 2
