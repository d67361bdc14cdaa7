"""The depthwise and fused depthwise -> 1x1 launch plans (paddle-lite_amd/csrc/dw_plan.h: kernel family, template parameters, the
argument block's launch-plan fields, grid, block, LDS for every problem and knob setting) against the recorded sweep
tests/golden/dw_plans/sweep.txt.  Stand-alone programs with their own main, compiled by g++ alone with
-fsanitize=address,undefined: the header takes no HIP.  The fixture was written from the launchers' own decision code before
dw_plan.h replaced it (tools/dump_dw_plans.py); moving any threshold of a plan changes a digest.  No device."""
import importlib.util
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dump_dw_plans", os.path.join(ROOT, "tools", "dump_dw_plans.py"))
dump = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump)
SANITIZE = ("-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")

# fusion G on every shape of a small grid, x aligned and not: where the aligned plan stages dwords, the misaligned one stages
# bytes (DWORD, wu, rpp move) and every other field of the plan's text stays; a byte-staged plan does not move at all.
MISALIGNED = r"""
#include <stdio.h>
#include <string>
#include "dw_plan.h"
int main() {
  long dword = 0, bytes = 0, bad = 0;
  for (int C : {16, 96, 1024})
    for (int M : {8, 128, 1024})
      for (int ow : {7, 14, 28, 56, 112, 130})
        for (int s = 1; s <= 2; ++s)
          for (int pl = 0; pl <= 1; ++pl)
            for (int extra = 0; extra < s; ++extra) {
              plhip::DwProblem q = {};
              q.n = 2; q.C = C; q.oh = q.ow = ow; q.h = q.w = (ow - 1) * s + 3 - 2 * pl + extra; q.kh = q.kw = 3; q.pt = q.pl = pl;
              q.sh = q.sw = s; q.dh = q.dw = 1; q.out = plhip::DW_OUT_F32; q.pw_M = M; q.x_aligned = true;
              plhip::DwPlan a = plhip::dw_conv1x1_launch_plan(q, plhip::DwKnobs());
              q.x_aligned = false;
              const plhip::DwPlan b = plhip::dw_conv1x1_launch_plan(q, plhip::DwKnobs());
              if (a.family != plhip::DW_CONV1X1 || b.family != plhip::DW_CONV1X1 || b.DWORD) { ++bad; continue; }
              if (a.DWORD != (q.w % 4 == 0)) ++bad;
              a.DWORD ? ++dword : ++bytes;
              if (a.DWORD) {  // the byte form of the same rows
                if (b.g.wu != a.g.WP || a.g.wu != a.g.WP / 4 || b.g.rpp != (b.g.wu <= 64 ? 64 / b.g.wu : 1)) ++bad;
                a.DWORD = false; a.g.wu = b.g.wu; a.g.rpp = b.g.rpp;
              }
              char ta[768], tb[768];
              plhip::dw_plan_text(a, ta, sizeof ta);
              plhip::dw_plan_text(b, tb, sizeof tb);
              if (std::string(ta) != tb) { if (bad++ < 5) printf("%s\n%s\n", ta, tb); }
            }
  printf("dword %ld bytes %ld bad %ld\n", dword, bytes, bad);
  return bad != 0 || dword == 0 || bytes == 0;
}
"""


@pytest.fixture(scope="module")
def swept():
    """The lines of the sanitised sweep program."""
    with tempfile.TemporaryDirectory(prefix="dw_plans.") as tmp:
        return dump.sweep(dump.build(tmp, flags=SANITIZE))


def test_plans_equal_the_recorded_sweep(swept):
    """A digest that differs names its group; `tools/dump_dw_plans.py --full DIR` on both trees shows the lines."""
    want = dump.load_fixture()
    assert len(want) == dump.GROUPS + 1
    for g, w in zip(swept, want):
        assert g == w, "the sweep group differs\n  dw_plan.h: %s\n  recorded : %s" % (g, w)
    assert len(swept) == len(want)


def test_sweep_reaches_every_plan_and_every_kernel_instance(swept):
    dump.check_cover(swept)
    dump.check_cover(dump.load_fixture())


def test_misaligned_input_only_turns_dword_staging_into_byte_staging():
    with tempfile.TemporaryDirectory(prefix="dw_misaligned.") as tmp:
        src, exe = os.path.join(tmp, "misaligned_main.cc"), os.path.join(tmp, "misaligned_main")
        with open(src, "w") as f:
            f.write(MISALIGNED)
        p = subprocess.run(["g++", "-std=c++17", "-Wall", *SANITIZE, "-I", dump.CSRC, src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert p.returncode == 0, "dw_plan.h does not compile alone:\n" + p.stdout.decode()[-3000:]
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
