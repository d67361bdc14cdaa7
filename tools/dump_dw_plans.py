#!/usr/bin/env python3
"""The depthwise and fused depthwise -> 1x1 launch plans (paddle-lite_amd/csrc/dw_plan.h) over a sweep of problems and knob
settings, as the text fixture tests/golden/dw_plans/sweep.txt (tests/test_dw_plan_host.py recomputes it and compares).

A stand-alone program (its own main, g++ alone, no device) includes dw_plan.h and prints, for every problem, one line

  n C h w oh ow kh kw pt pl sh sw dh dw out pw_M x_aligned | <dw_plan_text of its plan>

The fixture holds one line per (knob setting, kind, output kind): the count per plan name and a sha256 over the group's whole
lines, and a last line with the number of distinct kernel instances (template parameters and output kind) the sweep reached per
family.  `--full DIR` writes the whole lines, one file per (kind, knob setting), to diff two builds when a digest differs.

Kinds: dw (depthwise_launch_plan: 3x3, 5x5 and a dilated 3x3, stride 1 | 2, left / top pad 0..4, planes from 1 x 1 to 200 x 200
and two rows too wide for the band kernel's LDS; every (C, n) on the square planes), pairD (dwpw_launch_plan: every whitelisted shape, its near misses in C, M, plane
and pad, n at the 32-bit guards; the plane-average output too) and pairG (dw_conv1x1_launch_plan, x aligned and not).  Each kind
runs under its own knobs: the default, and every knob at every other value.

The fixture was first written from the launchers' own code before dw_plan.h replaced it; a refactor must leave it alone.  Rewrite
it (`python tools/dump_dw_plans.py`) only in a change that is meant to move a launch, and review the diff.  Writing checks that
every plan name and "none" occur and that every kernel instance a plan can name is reached."""
import argparse
import importlib.util
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "paddle-lite_amd", "csrc")
PLANS_DIR = os.path.join(ROOT, "tests", "golden", "dw_plans")
_spec = importlib.util.spec_from_file_location("dump_gemm_plans", os.path.join(ROOT, "tools", "dump_gemm_plans.py"))
_gemm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_gemm)

NAMES = ["dw_direct", "dw_band", "dw_generic", "dwpw_14x14", "dwpw_14x14_mtw2", "dwpw_stream", "dwpw_7x7", "dw_conv1x1", "none"]
# Kernel instances a plan can name, (template parameters, output kind), against the kernel symbols of the five files' gfx950 ISA:
#   dw_direct   96 of 144 built: KS 2 x S 2 x RS 3 x FASTV 2 x (int8: STAGE 2; int32, fp32: STAGE 0 only -- the 48 staged 32-bit
#               instances are built and never launched: staging is an int8 form)
#   dw_band     15 of 15: FAST 5 x OUT 3
#   dwpw_14x14   6 plans = 16 built with the executor's (DWNN, PWNN) split: MTW 2 x (int8: 4; int32, fp32: 2)
#   dwpw_stream 18 plans = 72 built: 6 shapes x OUT 3 (x 4 (DWNN, PWNN); PWNN with a 32-bit output is built and never launched)
#   dwpw_7x7    16 plans = 64 built: 2 shapes x MB 2 x OUT 4 (x 4, as above)
#   dw_conv1x1  96 plans = 48 built: NACC 4 x OUT 3 x S 2 x PL 2 (x dword / byte staging, a kernel argument)
INSTANCES = "instances dw_direct=96 dw_band=15 dwpw_14x14=6 dwpw_stream=18 dwpw_7x7=16 dw_conv1x1=96"
GROUPS = 12 * 3 + 12 * 4 + 2 * 3

# The includer defines Prob (the fields of DwProblem, in its order), Setting below and
# int plan_line(const Setting&, int kind, const Prob&, char* buf, size_t cap)  (dw_plan_text's line of the plan).
DRIVER = _gemm.PRELUDE + r"""
#include <stdlib.h>
enum { KIND_DW = 0, KIND_D = 1, KIND_G = 2 };
static const Setting kSettings[] = {
    //                            stage np2 fastv k5 rs1 rs2 fs small dwconv
    {"default", KIND_DW,              1, 1, 1, 1, 0, 0, 1, 1, 1}, {"DW_STAGE=0", KIND_DW,     0, 1, 1, 1, 0, 0, 1, 1, 1},
    {"DW_STAGE_NP2=0", KIND_DW,       1, 0, 1, 1, 0, 0, 1, 1, 1}, {"DW_STAGE_NP2=2", KIND_DW, 1, 2, 1, 1, 0, 0, 1, 1, 1},
    {"DW_FASTV=0", KIND_DW,           1, 1, 0, 1, 0, 0, 1, 1, 1}, {"DW5_DIRECT=0", KIND_DW,   1, 1, 1, 0, 0, 0, 1, 1, 1},
    {"DW_RS1=4", KIND_DW,             1, 1, 1, 1, 4, 0, 1, 1, 1}, {"DW_RS1=7", KIND_DW,       1, 1, 1, 1, 7, 0, 1, 1, 1},
    {"DW_RS1=8", KIND_DW,             1, 1, 1, 1, 8, 0, 1, 1, 1}, {"DW_RS2=4", KIND_DW,       1, 1, 1, 1, 0, 4, 1, 1, 1},
    {"DW_RS2=7", KIND_DW,             1, 1, 1, 1, 0, 7, 1, 1, 1}, {"DW_RS2=8", KIND_DW,       1, 1, 1, 1, 0, 8, 1, 1, 1},
    {"FUSED_STREAM=0,FUSED_SMALL=0", KIND_D, 1, 1, 1, 1, 0, 0, 0, 0, 1}, {"FUSED_STREAM=0,FUSED_SMALL=1", KIND_D, 1, 1, 1, 1, 0, 0, 0, 1, 1},
    {"FUSED_STREAM=0,FUSED_SMALL=2", KIND_D, 1, 1, 1, 1, 0, 0, 0, 2, 1}, {"FUSED_STREAM=1,FUSED_SMALL=0", KIND_D, 1, 1, 1, 1, 0, 0, 1, 0, 1},
    {"default", KIND_D,                      1, 1, 1, 1, 0, 0, 1, 1, 1}, {"FUSED_STREAM=1,FUSED_SMALL=2", KIND_D, 1, 1, 1, 1, 0, 0, 1, 2, 1},
    {"FUSED_STREAM=2,FUSED_SMALL=0", KIND_D, 1, 1, 1, 1, 0, 0, 2, 0, 1}, {"FUSED_STREAM=2,FUSED_SMALL=1", KIND_D, 1, 1, 1, 1, 0, 0, 2, 1, 1},
    {"FUSED_STREAM=2,FUSED_SMALL=2", KIND_D, 1, 1, 1, 1, 0, 0, 2, 2, 1}, {"FUSED_STREAM=3,FUSED_SMALL=0", KIND_D, 1, 1, 1, 1, 0, 0, 3, 0, 1},
    {"FUSED_STREAM=3,FUSED_SMALL=1", KIND_D, 1, 1, 1, 1, 0, 0, 3, 1, 1}, {"FUSED_STREAM=3,FUSED_SMALL=2", KIND_D, 1, 1, 1, 1, 0, 0, 3, 2, 1},
    {"default", KIND_G,               1, 1, 1, 1, 0, 0, 1, 1, 1}, {"DWCONV_FUSED=0", KIND_G,  1, 1, 1, 1, 0, 0, 1, 1, 0},
};
static const char* const kKinds[] = {"dw", "pairD", "pairG"};
static const char* const kOuts[] = {"i32", "f32", "i8", "gap"};
static const char* const kFams[] = {"dw_direct", "dw_band", "dwpw_14x14", "dwpw_stream", "dwpw_7x7", "dw_conv1x1"};
static const int kPlane[] = {1, 4, 5, 7, 8, 13, 14, 28, 56, 112, 200};

struct Group {
  sha::Ctx sha;
  std::map<std::string, long> count;
  long n = 0;
};
static long g_problems = 0;

// argv[1] (optional): a directory for the whole lines, one file per (kind, knob setting)
int main(int argc, char** argv) {
  std::set<std::string> instances[6];
  char line[1024];
  for (const Setting& st : kSettings) {
    const int kind = st.kind;
    FILE* full = nullptr;
    if (argc > 1) {
      std::string path = std::string(argv[1]) + "/" + kKinds[kind] + "." + st.name + ".txt";
      for (char& c : path) if (c == '=' || c == ',') c = '_';
      full = fopen(path.c_str(), "w");
      if (!full) return 2;
    }
    Group groups[4];
    std::string last[4];
    long* last_count[4] = {};
    const int nouts = kind == KIND_D ? 4 : 3;
    auto one = [&](Prob q) {  // the problem on every output kind
      for (int out = 0; out < nouts; ++out) {
        q.out = out;
        int n = snprintf(line, sizeof line, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d | ", q.n, q.C, q.h, q.w, q.oh, q.ow, q.kh, q.kw,
                         q.pt, q.pl, q.sh, q.sw, q.dh, q.dw, q.out, q.pw_M, (int)q.x_aligned);
        const char* plan = line + n;
        n += plan_line(st, kind, q, line + n, sizeof line - (size_t)n - 1);
        if (n < 0 || (size_t)n >= sizeof line - 1) exit(3);
        line[n++] = '\n';
        Group& g = groups[out];
        g.sha.add(line, (size_t)n);
        g.n++;
        ++g_problems;
        if (full) fwrite(line, 1, (size_t)n, full);
        // the plan's name and the kernel instance (the template parameters and the output kind), looked up when they change
        const char* end = strstr(plan, " grid=");
        const size_t len = end ? (size_t)(end - plan) : strcspn(plan, " ");
        if (len != last[out].size() || memcmp(plan, last[out].data(), len) != 0) {
          last[out].assign(plan, len);
          const std::string name(plan, strcspn(plan, " "));
          last_count[out] = &g.count[name];
          const std::string fam = name == "dw_generic" ? "dw_band" : name == "dwpw_14x14_mtw2" ? "dwpw_14x14" : name;
          for (int f = 0; f < 6; ++f)
            if (fam == kFams[f]) instances[f].insert(last[out] + " OUT=" + kOuts[out]);
        }
        ++*last_count[out];
      }
    };
    if (kind == KIND_DW) {
      static const int kKD[][2] = {{3, 1}, {5, 1}, {3, 2}};  // filter size, dilation
      static const int kC[] = {1, 3, 16, 24}, kN[] = {1, 2, 128};
      for (const auto& kd : kKD)
        for (int s = 1; s <= 2; ++s)
          for (int pl = 0; pl <= 4; ++pl)
            for (int far = 0; far < 2; ++far)  // bottom / right pad = top / left, or none with the input a row / column larger where the stride drops one
              for (int ih = 0; ih <= 12; ++ih)
                for (int iw = 0; iw < 11; ++iw) {
                  if (ih >= 11 && iw != 0) continue;
                  // the last two: a row too wide for the band kernel, and one whose 3x3 band lies between its two LDS bounds
                  const int oh = ih >= 11 ? 1 : kPlane[ih], ow = ih == 11 ? 24000 : ih == 12 ? 21000 : kPlane[iw];
                  const int keff = (kd[0] - 1) * kd[1] + 1;
                  const int h = (oh - 1) * s + keff - pl - (far ? 0 : pl) + (far ? s - 1 : 0), w = (ow - 1) * s + keff - pl - (far ? 0 : pl) + (far ? s - 1 : 0);
                  if (h < 1 || w < 1) continue;
                  for (int C : kC)
                    for (int n : kN) {
                      if (oh != ow && !(C == 24 && n == 2)) continue;  // every (C, n) on the square planes, one on the others
                      Prob q = Prob();
                      q.n = n; q.C = C; q.h = h; q.w = w; q.oh = oh; q.ow = ow; q.kh = q.kw = kd[0]; q.pt = q.pl = pl; q.sh = q.sw = s;
                      q.dh = q.dw = kd[1]; q.x_aligned = true;
                      one(q);
                    }
                }
    } else if (kind == KIND_D) {
      // (C, h, stride, M): the streaming kernel's six, the 7 x 7 kernel's two, the 14 x 14 kernel's eight
      static const int kShapes[][4] = {{32, 112, 1, 64},   {128, 56, 1, 128},  {256, 28, 1, 256},  {64, 112, 2, 128},  {128, 56, 2, 256},
                                       {256, 28, 2, 512},  {512, 14, 2, 1024}, {1024, 7, 1, 1024}, {128, 14, 1, 256},  {128, 14, 1, 512},
                                       {256, 14, 1, 256},  {256, 14, 1, 512},  {384, 14, 1, 256},  {384, 14, 1, 512},  {512, 14, 1, 256},
                                       {512, 14, 1, 512}};
      for (const auto& sh : kShapes)
        for (int var = 0; var < 12; ++var) {  // the shape itself, then its near misses
          int C = sh[0], h = sh[1], w = sh[1], s = sh[2], M = sh[3], pad = 1, k = 3, dil = 1, s2 = s;
          switch (var) {
            case 1: C -= 32; break;
            case 2: C += 32; break;
            case 3: C += 128; break;
            case 4: M /= 2; break;
            case 5: M *= 2; break;
            case 6: M += 32; break;
            case 7: h += s; break;  // not square
            case 8: pad = 0; break;
            case 9: k = 5; pad = 2; break;
            case 10: dil = 2; pad = 2; break;
            case 11: s2 = 3 - s; break;  // the two strides differ
          }
          const int keff = (k - 1) * dil + 1;
          const int oh = (h + 2 * pad - keff) / s + 1, ow = (w + 2 * pad - keff) / s2 + 1;
          if (oh < 1 || ow < 1 || C < 1) continue;
          const long g1 = (((long)1 << 31) - 65536) / ((long)C * h * w), g2 = ((long)1 << 31) / ((long)M * oh * ow);  // n at the 32-bit guards
          const long ns[] = {1, 2, 128, g1 - 1, g1, g1 + 1, g2 - 1, g2, g2 + 1};
          for (long n : ns) {
            if (n < 1 || n * 8 >= ((long)1 << 31)) continue;
            Prob q = Prob();
            q.n = (int)n; q.C = C; q.h = h; q.w = w; q.oh = oh; q.ow = ow; q.kh = q.kw = k; q.pt = q.pl = pad; q.sh = s; q.sw = s2;
            q.dh = q.dw = dil; q.pw_M = M; q.x_aligned = true;
            one(q);
          }
        }
    } else {
      static const int kC[] = {16, 32, 96, 384, 1024, 1040}, kM[] = {8, 64, 128, 256, 1024, 1032}, kOW[] = {7, 14, 28, 56, 112, 130}, kN[] = {1, 2, 128};
      for (int C : kC)
        for (int M : kM)
          for (int ow : kOW)
            for (int s = 1; s <= 2; ++s)
              for (int pl = 0; pl <= 1; ++pl)
                for (int al = 1; al >= 0; --al)
                  for (int n : kN) {
                    Prob q = Prob();
                    // (n = 2: the input a row and a column larger where the stride drops one)
                    q.n = n; q.C = C; q.oh = q.ow = ow; q.h = q.w = (ow - 1) * s + 3 - 2 * pl + (n == 2 ? s - 1 : 0); q.kh = q.kw = 3; q.pt = q.pl = pl;
                    q.sh = q.sw = s; q.dh = q.dw = 1; q.pw_M = M; q.x_aligned = al != 0;
                    one(q);
                  }
    }
    for (int out = 0; out < nouts; ++out) {
      Group& g = groups[out];
      printf("%s %s %s n=%ld", st.name, kKinds[kind], kOuts[out], g.n);
      for (const auto& kv : g.count) printf(" %s=%ld", kv.first.c_str(), kv.second);
      printf(" sha256=%s\n", g.sha.hex().c_str());
    }
    if (full) fclose(full);
  }
  fprintf(stderr, "%ld (problem, setting) pairs\n", g_problems);
  printf("instances");
  for (int f = 0; f < 6; ++f) printf(" %s=%zu", kFams[f], instances[f].size());
  printf("\n");
  return 0;
}
"""

# the program of this repository: Prob is DwProblem itself, the plans are dw_plan.h's
PROGRAM = r"""
#include "dw_plan.h"
typedef plhip::DwProblem Prob;
struct Setting { const char* name; int kind, stage, np2, fastv, k5, rs1, rs2, fs, fsmall, dwconv; };
static int plan_line(const Setting& st, int kind, const Prob& q, char* buf, size_t cap) {
  plhip::DwKnobs k;
  k.stage = st.stage; k.stage_np2 = st.np2; k.fastv = st.fastv; k.k5_direct = st.k5; k.rs1 = st.rs1; k.rs2 = st.rs2;
  k.fused_stream = st.fs; k.fused_small = st.fsmall; k.dwconv_fused = st.dwconv;
  const plhip::DwPlan p = kind == 0 ? plhip::depthwise_launch_plan(q, k) : kind == 1 ? plhip::dwpw_launch_plan(q, k) : plhip::dw_conv1x1_launch_plan(q, k);
  return plhip::dw_plan_text(p, buf, cap);
}
""" + DRIVER


def build(tmp, program=PROGRAM, flags=("-O2",)):
    """Compiles the sweep program with g++ alone; returns its path."""
    src, exe = os.path.join(tmp, "dw_plans_main.cc"), os.path.join(tmp, "dw_plans_main")
    with open(src, "w") as f:
        f.write(program)
    p = subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-I", CSRC, src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, "dw_plan.h does not compile alone:\n" + p.stdout.decode()[-3000:]
    return exe


def sweep(exe, full_dir=None):
    r = subprocess.run([exe] + ([full_dir] if full_dir else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, "the sweep program failed:\n" + r.stderr.decode()[-3000:]
    return r.stdout.decode().splitlines()


def check_cover(lines):
    """Every plan name and the none outcome occur; every kernel instance a plan can name is reached."""
    seen = {kv.split("=")[0] for ln in lines[:-1] for kv in ln.split()[4:-1]}
    assert seen == set(NAMES), sorted(seen ^ set(NAMES))
    assert lines[-1] == INSTANCES, lines[-1]


def load_fixture():
    with open(os.path.join(PLANS_DIR, "sweep.txt")) as f:
        return f.read().splitlines()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--full", metavar="DIR", help="also write the sweep's whole lines, one file per (kind, knob setting), to DIR")
    args = ap.parse_args()
    if args.full:
        os.makedirs(args.full, exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="dw_plans.") as tmp:
        lines = sweep(build(tmp), args.full)
    check_cover(lines)
    assert len(lines) == GROUPS + 1, len(lines)
    os.makedirs(PLANS_DIR, exist_ok=True)
    with open(os.path.join(PLANS_DIR, "sweep.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d groups -> %s" % (len(lines) - 1, PLANS_DIR))


if __name__ == "__main__":
    sys.exit(main())
