"""pack4_nn_rtz (plhip_device.h) switches MODE.fp_round to round-toward-zero and back with s_setreg inside inline asm.  LLVM's
hazard recogniser does not look inside inline asm, so two inlined expansions must not leave two MODE writes back to back:
in every kept ISA file (csrc/*-gfx950.s) at least two instructions separate consecutive MODE writes.  The scan follows the
text order of the ISA: it checks straight-line adjacency only (two writes that meet across a branch are not seen)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "paddle-lite_amd", "csrc")
_INS = re.compile(r"^\s+([a-z_][a-z0-9_]*)\b")  # an instruction line (labels, directives and comments do not match)
_MODE = re.compile(r"^\s+s_setreg\w*\s+hwreg\((HW_REG_MODE|1)\b")


def _close_mode_writes(text, gap=2):
    found, last, idx = [], None, 0
    for ln, line in enumerate(text.splitlines(), 1):
        if line.lstrip().startswith((".", ";", "//")) or not _INS.match(line):
            continue
        if re.match(r"^\s*\S+:", line):
            continue
        idx += 1
        if _MODE.match(line):
            if last is not None and idx - last[0] <= gap:
                found.append((last[1], ln))
            last = (idx, ln)
    return found


def test_no_back_to_back_mode_writes():
    files = sorted(glob.glob(os.path.join(CSRC, "*-gfx950.s")))
    assert len(files) == len(glob.glob(os.path.join(CSRC, "*.hip"))), "build the library first (one kept ISA file per unit)"
    bad, total = {}, 0
    for f in files:
        text = open(f).read()
        total += len(re.findall(r"s_setreg\w*\s+hwreg\(HW_REG_MODE", text))
        close = _close_mode_writes(text)
        if close:
            bad[os.path.basename(f)] = close[:4]
    assert total > 0, "no MODE write found: pack4_nn_rtz changed, revisit this test"
    assert not bad, bad


def test_the_scan_sees_adjacent_writes():
    text = ("\ts_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0\n\tv_mov_b32 v0, v1\n"
            "\ts_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3\n")
    assert _close_mode_writes(text) == [(1, 3)]
    assert _close_mode_writes(text.replace("\tv_mov_b32 v0, v1\n", "\tv_mov_b32 v0, v1\n\ts_nop 0\n")) == []
