"""tools/isa_diff.py (the comparison of two builds' kept gfx950 ISA) on three synthetic units, one per verdict.  No device."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_diff", os.path.join(ROOT, "tools", "isa_diff.py"))
isa_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_diff)

# the shape of what -save-temps=obj keeps: a function between its .type line and .Lfunc_end, its kernel descriptor, its entry
# in the metadata (an argument's .name sits deeper than the kernel's)
UNIT = """\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"
\t.type\tkern_a,@function
kern_a:                                 ; @kern_a
; %bb.0:
\ts_load_dword s3, s[0:1], 0x30
\tv_cvt_f32_i32_e32 {r}, v0              ; a comment
\tv_fma_f32 {r}, {r}, v2, v3
{extra}\ts_cbranch_execz .LBB0_{lab}
.LBB0_{lab}:                                ; %Flow
\ts_endpgm
.Lfunc_end0:
\t.size\tkern_a, .Lfunc_end0-kern_a
\t.amdhsa_kernel kern_a
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 16
\t.end_amdhsa_kernel
\t.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .address_space:  global
        .name:           x
        .size:           8
    .group_segment_fixed_size: 0
    .name:           kern_a
    .private_segment_fixed_size: 0
    .sgpr_count:     22
    .sgpr_spill_count: 0
    .symbol:         kern_a.kd
    .vgpr_count:     {vgpr}
    .vgpr_spill_count: 0
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
...
\t.end_amdgpu_metadata
"""


def unit(r="v1", lab=2, vgpr=4, extra=""):
    return UNIT.format(r=r, lab=lab, vgpr=vgpr, extra=extra)


def test_parse_takes_instructions_and_resource_lines_only():
    ins, res = isa_diff.parse(unit())["kern_a"]
    assert ins == ["s_load_dword s3, s[0:1], 0x30", "v_cvt_f32_i32_e32 v1, v0", "v_fma_f32 v1, v1, v2, v3", "s_cbranch_execz .LBB0_2",
                   "s_endpgm"]
    assert res == ["agpr_count 0", "amdhsa_next_free_sgpr 16", "amdhsa_next_free_vgpr 4", "group_segment_fixed_size 0",
                   "private_segment_fixed_size 0", "sgpr_count 22", "sgpr_spill_count 0", "vgpr_count 4", "vgpr_spill_count 0"]
    assert list(isa_diff.parse(unit())) == ["kern_a"]  # (the metadata's keys are no symbols)


def test_identical():
    old = unit()
    new = old.replace("; a comment", "; another comment").replace("; %Flow", "; %Flow77")
    assert isa_diff.compare(old, new) == ("identical", [])


def test_renamed():
    # another register, another block label: the same mnemonics and the same resources
    assert isa_diff.compare(unit(), unit(r="v5", lab=7)) == ("renamed", [])


def test_different_instructions():
    verdict, out = isa_diff.compare(unit(), unit(extra="\tv_max_f32_e32 v1, v1, v1\n\ts_nop 0\n"))
    assert verdict == "different"
    assert len(out) == 1 and "kern_a" in out[0] and "+2 instructions" in out[0] and "+1 s_nop" in out[0] and "+1 v_max_f32_e32" in out[0]


def test_different_resources_alone():
    verdict, out = isa_diff.compare(unit(), unit(vgpr=5))
    assert verdict == "different"
    assert "+0 instructions" in out[0] and "amdhsa_next_free_vgpr 4 -> 5" in out[0] and "vgpr_count 4 -> 5" in out[0]


def test_a_kernel_in_one_build_only_is_different():
    verdict, out = isa_diff.compare(unit(), unit().replace("kern_a", "kern_b"))
    assert verdict == "different" and len(out) == 2


def test_main_walks_two_directories(tmp_path, capsys):
    for d, texts in (("old", (unit(), unit(), unit())), ("new", (unit(), unit(r="v9"), unit(vgpr=6)))):
        os.mkdir(tmp_path / d)
        for name, t in zip(("same", "regs", "more"), texts):
            (tmp_path / d / (name + "-hip-amdgcn-amd-amdhsa-gfx950.s")).write_text(t)
    assert isa_diff.main(str(tmp_path / "old"), str(tmp_path / "new")) == 1
    lines = capsys.readouterr().out.splitlines()
    assert [l.split() for l in lines if not l.startswith(" ")] == [["more", "different"], ["regs", "renamed"], ["same", "identical"]]
