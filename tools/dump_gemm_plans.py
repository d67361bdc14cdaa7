#!/usr/bin/env python3
"""The GEMM launch plans (paddle-lite_amd/csrc/gemm_plan.h) over a sweep of problems and knob settings, as the text fixture
tests/golden/gemm_plans/sweep.txt (tests/test_gemm_plan_host.py recomputes it and compares).

A stand-alone program (its own main, g++ alone, no device) includes gemm_plan.h and prints, for every problem, one line

  M K KS HWX HWY XP NB im_kw im_s res y2 y out ma vec_store aligned | name family=.. MA=.. ... grid=.. block=.. lds=..

i.e. the GemmProblem and gemm_plan_text of its plan.  The fixture holds one line per (knob setting, operand kind, output kind): the
count per plan name and a sha256 over the group's whole lines, and a last line with the number of distinct kernel instances the
sweep reached per family.  `--full DIR` writes the whole lines, one file per knob setting, to diff two builds when a digest differs.

The sweep is the product of SWEEP's axes.  Operand kinds: a dense NCHW slab (XP = HW, HWX = HW rounded up to 4), an im2col buffer
(XP = HWX), and the implicit GEMM at stride 1 and 2 (an image = one output row of OW columns, OH = OW).  ma, vec_store and aligned
as plhip_capi_conv.hip passes them for aligned pointers; the dense slab (the one operand that can arrive misaligned) also with
aligned = false.  A tail exists with fp32 output only.

The fixture was first written from the launchers' own code before gemm_plan.h replaced it; a refactor must leave it alone.  Rewrite
it (`python tools/dump_gemm_plans.py`) only in a change that is meant to move a launch, and review the diff.  Writing checks that
every plan name and "none" occur and that every kernel instance the library builds for these families is reached."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "paddle-lite_amd", "csrc")
PLANS_DIR = os.path.join(ROOT, "tests", "golden", "gemm_plans")
NAMES = ["gemm_nchw", "gemm_vperm_lds", "gemm_ring", "gemm_ring_ma1", "gemm_areg", "gemm_wide_n4", "gemm_wide_n7", "gemm_wide_n8",
         "gemm_tr_1x4", "gemm_tr_2x4", "gemm_tr_2x2", "gemm_tr_4x2", "gemm_tr_4x1", "none"]
# kernel instances the library builds (template-parameter combinations the plan names; the wide kernel's NONNEG follows the
# activation, which no plan reads): private and LDS 2 MA x 3 OUT x 4 store forms; ring 2 x 3 x 4 and 4 NG x 2 VS x 3 OUT of the
# register-ring form; tr 5 tiles x 3 OUT x 2 IM; wide (4 + 3 + 3) (NTT, KS) x 3 OUT
INSTANCES = "instances private=24 lds=24 ring=48 tr=30 wide=30"

# Shared by every program that prints a sweep (tools/dump_dw_plans.py too): the includes and SHA-256.
PRELUDE = r"""
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <map>
#include <set>
#include <string>
#include <vector>

// the driver's own hot loops stay uninstrumented in a sanitised build: the code under test is the includer's plan_rec
#define NOSAN __attribute__((no_sanitize("address", "undefined")))
namespace sha {  // SHA-256 (FIPS 180-4)
static const uint32_t K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
struct Ctx {
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  uint8_t buf[64];
  uint64_t n = 0;
  static uint32_t rot(uint32_t x, int r) { return (x >> r) | (x << (32 - r)); }
  NOSAN void block(const uint8_t* p) {
    uint32_t w[64], a[8];
    for (int i = 0; i < 16; ++i) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
    for (int i = 16; i < 64; ++i)
      w[i] = w[i - 16] + (rot(w[i - 15], 7) ^ rot(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] + (rot(w[i - 2], 17) ^ rot(w[i - 2], 19) ^ (w[i - 2] >> 10));
    memcpy(a, h, sizeof a);
    for (int i = 0; i < 64; i += 8) {  // the eight registers rotate by renaming
#define ROUND(A, B, C, D, E, F, G, H, I)                                                                      \
  {                                                                                                           \
    const uint32_t t1 = H + (rot(E, 6) ^ rot(E, 11) ^ rot(E, 25)) + ((E & F) ^ (~E & G)) + K[I] + w[I];          \
    D += t1;                                                                                                  \
    H = t1 + (rot(A, 2) ^ rot(A, 13) ^ rot(A, 22)) + ((A & B) ^ (A & C) ^ (B & C));                             \
  }
      ROUND(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], i)
      ROUND(a[7], a[0], a[1], a[2], a[3], a[4], a[5], a[6], i + 1)
      ROUND(a[6], a[7], a[0], a[1], a[2], a[3], a[4], a[5], i + 2)
      ROUND(a[5], a[6], a[7], a[0], a[1], a[2], a[3], a[4], i + 3)
      ROUND(a[4], a[5], a[6], a[7], a[0], a[1], a[2], a[3], i + 4)
      ROUND(a[3], a[4], a[5], a[6], a[7], a[0], a[1], a[2], i + 5)
      ROUND(a[2], a[3], a[4], a[5], a[6], a[7], a[0], a[1], i + 6)
      ROUND(a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[0], i + 7)
#undef ROUND
    }
    for (int i = 0; i < 8; ++i) h[i] += a[i];
  }
  NOSAN void add(const void* data, size_t len) {
    const uint8_t* p = (const uint8_t*)data;
    while (len) {
      const size_t at = n & 63, take = len < 64 - at ? len : 64 - at;
      memcpy(buf + at, p, take);
      n += take; p += take; len -= take;
      if ((n & 63) == 0) block(buf);
    }
  }
  std::string hex() {
    const uint64_t bits = n * 8;
    const uint8_t one = 0x80, zero = 0;
    add(&one, 1);
    while ((n & 63) != 56) add(&zero, 1);
    for (int i = 7; i >= 0; --i) {
      const uint8_t b = (uint8_t)(bits >> (8 * i));
      add(&b, 1);
    }
    char out[65];
    for (int i = 0; i < 8; ++i) snprintf(out + 8 * i, 9, "%08x", h[i]);
    return out;
  }
};
}  // namespace sha
"""

# The includer defines Prob (the fields of GemmProblem, in its order), Setting and Rec below and
# void plan_rec(const Setting&, const Prob&, Rec*)  (the plan's fields; the driver prints them as gemm_plan_text does).
DRIVER = PRELUDE + r"""
static const Setting kSettings[] = {
    //                     variant areg ma tr cfg wide ntt_knob ntt_override
    {"default",                  0, 1, 0, 1, 3, 1, 0, -1}, {"GEMM_VARIANT=1",           1, 1, 0, 1, 3, 1, 0, -1},
    {"GEMM_VARIANT=2",           2, 1, 0, 1, 3, 1, 0, -1}, {"GEMM_VARIANT=3",           3, 1, 0, 1, 3, 1, 0, -1},
    {"GEMM_AREG=0",              0, 0, 0, 1, 3, 1, 0, -1}, {"GEMM_VARIANT=3,GEMM_AREG=0", 3, 0, 0, 1, 3, 1, 0, -1},
    {"GEMM_MA=1",                0, 1, 1, 1, 3, 1, 0, -1}, {"GEMM_TR=0",                0, 1, 0, 0, 3, 1, 0, -1},
    {"GEMM_TR=2",                0, 1, 0, 2, 3, 1, 0, -1}, {"TR_CFG=0",                 0, 1, 0, 1, 0, 1, 0, -1},
    {"GEMM_TR=2,TR_CFG=0",       0, 1, 0, 2, 0, 1, 0, -1}, {"GEMM_WIDE=0",              0, 1, 0, 1, 3, 0, 0, -1},
    {"WIDE_NTT=4",               0, 1, 0, 1, 3, 1, 4, -1}, {"WIDE_NTT=7",               0, 1, 0, 1, 3, 1, 7, -1},
    {"WIDE_NTT=8",               0, 1, 0, 1, 3, 1, 8, -1}, {"override=4",               0, 1, 0, 1, 3, 1, 0, 4},
    {"override=7",               0, 1, 0, 1, 3, 1, 0, 7},  {"override=8",               0, 1, 0, 1, 3, 1, 0, 8},
    {"override=0",               0, 1, 0, 1, 3, 1, 0, 0},  {"override=0,WIDE_NTT=7",    0, 1, 0, 1, 3, 1, 7, 0},
};
static const int kM[] = {8, 32, 33, 64, 65, 96, 128, 129, 144, 160, 200, 256, 257, 300, 512, 1024};
static const int kK[] = {16, 32, 64, 96, 128, 160, 256, 512, 1024, 1088};
static const int kPlane[] = {16, 17, 20, 36, 49, 196, 784, 3136};
static const int kNB[] = {1, 2, 128};
static const int kKhkw[] = {9, 25, 49};
static const int kOW[] = {7, 14, 16, 56};
static const char* const kKinds[] = {"dense", "im2col", "implicit_s1", "implicit_s2"};
static const char* const kOuts[] = {"i32", "f32", "i8"};

struct Group {
  sha::Ctx sha;
  std::map<std::string, long> count;
  long n = 0;
};
// snprintf is most of the run time at four million lines
NOSAN static char* put(char* o, const char* s) { while (*s) *o++ = *s++; return o; }
NOSAN static char* put(char* o, unsigned long v) {
  char t[24];
  int n = 0;
  do t[n++] = (char)('0' + v % 10); while (v /= 10);
  while (n) *o++ = t[--n];
  return o;
}
NOSAN static char* put(char* o, const char* key, unsigned long v) { return put(put(o, key), v); }

// argv[1] (optional): a directory for the whole lines, one file per knob setting
int main(int argc, char** argv) {
  static const char* const kFams[] = {"none", "private", "lds", "ring", "tr", "wide"};
  std::set<std::string> instances[6];
  std::string key, last_key[6], last_name;
  char line[768];
  for (const Setting& st : kSettings) {
    FILE* full = nullptr;
    if (argc > 1) {
      std::string path = std::string(argv[1]) + "/" + st.name + ".txt";
      for (char& c : path) if (c == '=' || c == ',') c = '_';
      full = fopen(path.c_str(), "w");
      if (!full) return 2;
    }
    for (int kind = 0; kind < 4; ++kind) {
      Group groups[3];
      Group* last_group = nullptr;
      long* g_count = nullptr;
      last_name.clear();
      auto one = [&](Prob p) {
        for (int out = 0; out < 3; ++out) {
          for (int tail = 0; tail < (out == 1 ? 3 : 1); ++tail) {  // none / residual / int8 copy only (the fp32 output dropped)
            for (int al = 0; al < (kind == 0 ? 2 : 1); ++al) {  // the caller's flags for aligned pointers; a dense slab: then a misaligned one
              Prob q = p;
              q.out = out;
              q.res = tail == 1;
              q.y2 = tail == 2;
              q.y = tail != 2;
              if (al) q.aligned_loads = false;
              Rec r = Rec();
              plan_rec(st, q, &r);
              const int v[16] = {q.M, q.K, q.KS, q.HWX, q.HWY, q.XP, q.NB, q.im_kw, q.im_s, q.res, q.y2, q.y, q.out, q.ma, q.vec_store, q.aligned_loads};
              char* o = line;
              for (int x : v) o = put(put(o, (unsigned long)x), " ");
              o = put(o, "| ");
              o = put(put(put(o, r.name), " family="), kFams[r.family]);
              const char* inst = o;  // the kernel instance: the template parameters, and the wide kernel's KS
              o = put(o, " MA=", r.MA); o = put(o, " OUT=", r.OUT); o = put(o, " VS=", r.VS); o = put(o, " MF=", r.MF); o = put(o, " AL=", r.AL);
              o = put(o, " NG=", r.NG); o = put(o, " WN=", r.WN); o = put(o, " WM=", r.WM); o = put(o, " D=", r.D); o = put(o, " IM=", r.IM);
              o = put(o, " NTT=", r.NTT);
              const char* inst_end = o;
              o = put(o, " HWX=", r.HWX); o = put(o, " MT=", r.MT); o = put(o, " NT=", r.NT); o = put(o, " grid=", r.grid);
              o = put(o, " block=", r.block); o = put(o, " lds=", r.lds);
              *o++ = '\n';
              Group& g = groups[out];
              g.sha.add(line, (size_t)(o - line));
              if (&g != last_group || last_name != r.name) g_count = &(last_group = &g)->count[last_name = r.name];
              ++*g_count;
              g.n++;
              if (full) fwrite(line, 1, (size_t)(o - line), full);
              if (r.family) {
                key.assign(inst, inst_end);
                if (r.family == 5) key += " KS=" + std::to_string(q.KS);
                if (key != last_key[r.family]) instances[r.family].insert(last_key[r.family] = key);
              }
            }
          }
        }
      };
      for (int M : kM)
        for (int K : kK)
          for (int nb : kNB) {
            Prob p = Prob();
            p.M = M; p.K = K; p.KS = (K + 31) / 32;
            p.ma = M > 32 ? 2 : 1;
            if (kind < 2) {
              for (int hw : kPlane) {
                const int np = (hw + 3) & ~3;
                p.HWX = np; p.HWY = hw; p.XP = kind == 0 ? hw : np; p.NB = nb; p.im_kw = 0; p.im_s = 1;
                p.vec_store = np == hw;
                p.aligned_loads = kind == 1 || (hw & 3) == 0;
                one(p);
              }
            } else {
              for (int khkw : kKhkw)
                for (int ow : kOW) {
                  p.HWX = ow; p.HWY = ow * ow; p.XP = 0; p.NB = nb * ow;
                  p.im_kw = khkw == 9 ? 3 : khkw == 25 ? 5 : 7; p.im_s = kind == 2 ? 1 : 2;
                  p.vec_store = (ow & 3) == 0;
                  p.aligned_loads = true;
                  one(p);
                }
            }
          }
      for (int out = 0; out < 3; ++out) {
        Group& g = groups[out];
        printf("%s %s %s n=%ld", st.name, kKinds[kind], kOuts[out], g.n);
        for (const auto& kv : g.count) printf(" %s=%ld", kv.first.c_str(), kv.second);
        printf(" sha256=%s\n", g.sha.hex().c_str());
      }
    }
    if (full) fclose(full);
  }
  printf("instances private=%zu lds=%zu ring=%zu tr=%zu wide=%zu\n", instances[1].size(), instances[2].size(), instances[3].size(),
         instances[4].size(), instances[5].size());
  return 0;
}
"""

# the program of this repository: Prob is GemmProblem itself, the plan is gemm_plan's
PROGRAM = r"""
#include "gemm_plan.h"
typedef plhip::GemmProblem Prob;
struct Setting { const char* name; int variant, areg, ma, tr, tr_cfg, wide, ntt_knob, ntt_override; };
struct Rec { int family; char name[24]; int MA, OUT, VS, MF, AL, NG, WN, WM, D, IM, NTT, HWX, MT, NT; unsigned grid, block; size_t lds; };
static void plan_rec(const Setting& st, const Prob& q, Rec* r) {
  plhip::GemmKnobs k;
  k.variant = st.variant; k.areg = st.areg; k.ma = st.ma; k.tr = st.tr; k.tr_cfg = st.tr_cfg; k.wide = st.wide;
  plhip::gemm_resolve_wide_force(&k, st.ntt_override, st.ntt_knob);
  const plhip::GemmPlan p = plhip::gemm_plan(q, k);
  *r = Rec{p.family, "", p.MA, p.OUT, p.VEC_STORE, p.MFULL, p.ALIGNED, p.NG, p.WN, p.WM, p.D, p.IM, p.NTT, p.HWX, p.MT, p.NT, p.grid, p.block, p.lds};
  memcpy(r->name, p.name, sizeof r->name);
}
""" + DRIVER


def build(tmp, program=PROGRAM, flags=("-O2",)):
    """Compiles the sweep program with g++ alone; returns its path."""
    src, exe = os.path.join(tmp, "gemm_plans_main.cc"), os.path.join(tmp, "gemm_plans_main")
    with open(src, "w") as f:
        f.write(program)
    p = subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-I", CSRC, src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, "gemm_plan.h does not compile alone:\n" + p.stdout.decode()[-3000:]
    return exe


def sweep(exe, full_dir=None):
    r = subprocess.run([exe] + ([full_dir] if full_dir else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, "the sweep program failed:\n" + r.stderr.decode()[-3000:]
    return r.stdout.decode().splitlines()


def check_cover(lines):
    """Every plan name and the none outcome occur; every kernel instance the library builds is reached."""
    seen = {kv.split("=")[0] for ln in lines[:-1] for kv in ln.split()[4:-1]}
    assert seen == set(NAMES), sorted(seen ^ set(NAMES))
    assert lines[-1] == INSTANCES, lines[-1]


def load_fixture():
    with open(os.path.join(PLANS_DIR, "sweep.txt")) as f:
        return f.read().splitlines()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--full", metavar="DIR", help="also write the sweep's whole lines, one file per knob setting, to DIR")
    args = ap.parse_args()
    if args.full:
        os.makedirs(args.full, exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="gemm_plans.") as tmp:
        lines = sweep(build(tmp), args.full)
    check_cover(lines)
    os.makedirs(PLANS_DIR, exist_ok=True)
    with open(os.path.join(PLANS_DIR, "sweep.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d groups -> %s" % (len(lines) - 1, PLANS_DIR))


if __name__ == "__main__":
    sys.exit(main())
