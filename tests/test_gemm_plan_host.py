"""The GEMM launch plan (paddle-lite_amd/csrc/gemm_plan.h: kernel family, template parameters, grid, block, LDS for every problem and
knob setting) against the recorded sweep tests/golden/gemm_plans/sweep.txt, and the host half of the magic-number division
(fastdiv_magic, csrc/dw_common.h).  Stand-alone programs with their own main, compiled by g++ alone with
-fsanitize=address,undefined: the headers take no HIP.  The fixture was written from the launchers' own decision code before
gemm_plan.h replaced it (tools/dump_gemm_plans.py); moving any threshold of the plan changes a digest.  No device."""
import importlib.util
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dump_gemm_plans", os.path.join(ROOT, "tools", "dump_gemm_plans.py"))
dump = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump)
SANITIZE = ("-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")

# fastdiv_magic's pair for every d in 1 .. 2^20 and 2^k, 2^k +- 1 up to 2^30: equal to the definition (power of two: magic 0,
# shift log2 d; else floor(2^(31 + l) / d) + 1 with l = ceil(log2 d), shift l - 1), and fastdiv_u31's formula on it divides
# exactly at 0, around multiples of d and at 2^31 - 1.
FASTDIV = r"""
#include <stdint.h>
#include <stdio.h>
#include "dw_common.h"
static uint32_t div_u31(uint32_t n, uint32_t magic, int sh) { return magic ? (uint32_t)(((uint64_t)n * magic) >> 32) >> sh : n >> sh; }
static long bad = 0, checked = 0;
static void check(long d) {
  unsigned m = 77;
  int sh = -77;
  plhip::fastdiv_magic(d, m, sh);
  int l = 0;
  while ((1L << l) < d) ++l;
  const bool pow2 = (1L << l) == d;
  const unsigned want_m = pow2 ? 0u : (unsigned)(((1ULL << (31 + l)) / (unsigned long long)d) + 1ULL);
  const int want_sh = pow2 ? l : l - 1;
  if (m != want_m || sh != want_sh) { if (bad++ < 5) printf("pair of %ld: %u %d, want %u %d\n", d, m, sh, want_m, want_sh); }
  const uint32_t top = 0x7fffffffu;
  const uint32_t q = top / (uint32_t)d;
  const uint32_t ns[] = {0, 1, (uint32_t)d - 1, (uint32_t)d, (uint32_t)d + 1, q / 2 * (uint32_t)d, q / 2 * (uint32_t)d + (uint32_t)d - 1,
                         q * (uint32_t)d - 1, q * (uint32_t)d, top - 1, top};
  for (uint32_t n : ns)
    if (n <= top && div_u31(n, m, sh) != n / (uint32_t)d) { if (bad++ < 5) printf("%u / %ld: %u\n", n, d, div_u31(n, m, sh)); }
  ++checked;
}
int main() {
  for (long d = 1; d <= (1L << 20); ++d) check(d);
  for (int k = 1; k <= 30; ++k) { check((1L << k) - 1 > 0 ? (1L << k) - 1 : 1); check(1L << k); if (k < 30) check((1L << k) + 1); }
  printf("checked %ld bad %ld\n", checked, bad);
  return bad != 0;
}
"""


@pytest.fixture(scope="module")
def swept():
    """The lines of the sanitised sweep program."""
    with tempfile.TemporaryDirectory(prefix="gemm_plans.") as tmp:
        return dump.sweep(dump.build(tmp, flags=SANITIZE))


def test_plans_equal_the_recorded_sweep(swept):
    """A digest that differs names its group; `tools/dump_gemm_plans.py --full DIR` on both trees shows the lines."""
    want = dump.load_fixture()
    assert len(want) == 20 * 4 * 3 + 1
    for g, w in zip(swept, want):
        assert g == w, "the sweep group differs\n  gemm_plan.h: %s\n  recorded   : %s" % (g, w)
    assert len(swept) == len(want)


def test_sweep_reaches_every_plan_and_every_kernel_instance(swept):
    dump.check_cover(swept)
    dump.check_cover(dump.load_fixture())


def test_fastdiv_magic_is_the_exact_pair():
    with tempfile.TemporaryDirectory(prefix="fastdiv.") as tmp:
        src, exe = os.path.join(tmp, "fastdiv_main.cc"), os.path.join(tmp, "fastdiv_main")
        with open(src, "w") as f:
            f.write(FASTDIV)
        p = subprocess.run(["g++", "-std=c++17", *SANITIZE, "-I", dump.CSRC, src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert p.returncode == 0, "dw_common.h's host half does not compile alone:\n" + p.stdout.decode()[-3000:]
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0 and r.stdout.decode().splitlines()[-1] == "checked %d bad 0" % ((1 << 20) + 89), r.stdout.decode()[-2000:]
