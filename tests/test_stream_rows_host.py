"""The staged produce of the streaming fused dw -> pw kernel (paddle-lite_amd/csrc/stream_rows.h: which 16-byte piece a lane
fetches, where its bytes go in the wave-private LDS stage, where a lane reads its windows) walked on the host: a stand-alone
program with its own main, compiled by g++ alone with -fsanitize=address,undefined.  For the four shapes the form exists for
(112 and 56 wide at stride 1, 56 and 28 wide at stride 2, whichever of them dw_plan.h switches on), n = 1 and n = 3, every
tile, wave, iteration, load and lane, composed the way fused_dwpw_stream.hip composes them (load 0's per-lane offsets of
iteration 0 + wave-uniform steps; the ragged last load's and the surplus iteration's own):
  * every fetched 16 bytes lie inside the tensor, and a lane with a piece fetches what task / group_src / piece_src say;
  * stage writes stay inside the wave's stage and touch no pad byte;
  * after the writes of an iteration on a position-coded tensor every window of every (group, input row, quad) is the window
    of the zero-padded tensor; a row outside the image holds other bytes and is one whose filter row the kernel zeroes.
No device."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "paddle-lite_amd", "csrc")
SANITIZE = ("-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")

WALK = r"""
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "dw_plan.h"
#include "stream_rows.h"
using plhip::stream_rows::LanePiece;
using plhip::stream_rows::Rows;
using plhip::stream_rows::Task;

static long bad = 0;
#define CHECK(c, ...) do { if (!(c)) { if (bad++ < 10) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint8_t code(long o) { return (uint8_t)(1 + (uint32_t)(o * 2654435761u >> 11) % 255u); }  // position code, never 0

int main() {
  long shapes = 0, fetches = 0, pieces = 0, writes = 0, windows = 0, outside = 0, clamped = 0;
  for (const plhip::dw_plan_detail::StreamShape& t : plhip::dw_plan_detail::kStreamShapes) {
    const bool has_form = (t.S == 1 && (t.W == 112 || t.W == 56)) || (t.S == 2 && (t.W == 56 || t.W == 28));
    CHECK(has_form || !t.ROWS, "W %d S %d staged without a geometry", t.W, t.S);
    if (!has_form) continue;
    ++shapes;
    const Rows R = {t.W, t.S, t.K, t.RS, t.TP};
    CHECK(R.ok(), "W %d S %d", t.W, t.S);
    const int H = t.W, HI = t.S * H, WI = R.WI(), TR = t.TP / t.W, NT = (H + TR - 1) / TR, G = R.G(), NL = R.NL(), U = R.U();
    for (int n : {1, 3}) {
      const long total = (long)n * t.K * HI * WI;
      std::vector<uint8_t> x(total);
      for (long o = 0; o < total; ++o) x[o] = code(o);
      for (int b = 0; b < n; ++b)
        for (int ti = 0; ti < NT; ++ti)
          for (int wave = 0; wave < 4; ++wave) {
            const int tr0 = ti * TR;
            std::vector<uint8_t> st(R.WB(), 0xAA), pad(R.WB(), 0);
            for (int g = 0; g < G; ++g)
              for (int k = 0; k <= R.NIN(); ++k)
                for (int i = 0; i < U; ++i) {
                  const int o = R.pad_off(g, k) + i;
                  CHECK(o >= 0 && o < R.WB(), "pad %d %d", g, k);
                  st[o] = 0;
                  pad[o] = 1;
                }
            for (int it = 0; it < R.NIT(); ++it) {
              const int gi0 = (it * 4 + wave) * G;
              const bool surplus = (it + 1) * 4 * G > R.NGRP();
              const long base = R.wave_base(b, gi0, tr0, H);
              for (int l = 0; l < NL; ++l)
                for (int lane = 0; lane < 64; ++lane) {
                  // the kernel's composition
                  const LanePiece lp = R.lane_piece(wave * G, lane, 0, tr0, H, false), lr = R.lane_piece(wave * G, lane, NL - 1, tr0, H, false);
                  const bool rl = R.ragged() && l == NL - 1;
                  long src;
                  if (surplus) src = base + R.lane_piece(gi0, lane, l, tr0, H).off;
                  else if (rl) src = base + lr.off;
                  else src = base + (long)l * R.src_step(H) + lp.off;
                  int dst[2];
                  for (int e = 0; e < R.UPP(); ++e) dst[e] = rl ? lr.dst[e] : lp.dst[e] + l * R.dst_step();
                  ++fetches;
                  CHECK(src >= 0 && src + 16 <= total, "fetch [%ld, +16) of %ld: W %d S %d n %d b %d tile %d wave %d it %d l %d lane %d", src, total,
                        t.W, t.S, n, b, ti, wave, it, l, lane);
                  CHECK(src % 16 == 0, "aligned %ld", src);
                  if (src < 0 || src + 16 > total) continue;
                  // what the geometry says of this lane's (group, piece)
                  const int g = l * R.GPL() + lane / R.NPGP(), j = lane % R.NPGP();
                  const bool has = g < G && j < R.NPG();
                  if (has) {
                    const Task tk = R.task(gi0 + g, tr0, H);
                    ++pieces;
                    clamped += gi0 + g >= R.NGRP();
                    CHECK(src == R.group_src(b, tk, H) + R.piece_src(j, tk), "piece: W %d S %d tile %d wave %d it %d l %d lane %d", t.W, t.S, ti, wave,
                          it, l, lane);
                    for (int e = 0; e < R.UPP(); ++e) CHECK(dst[e] == R.unit_dst(g, R.piece_unit(j) + e), "unit: W %d S %d l %d lane %d", t.W, t.S, l, lane);
                  }
                  for (int e = 0; e < R.UPP(); ++e) {
                    CHECK(dst[e] >= 0 && dst[e] + U <= R.WB() && dst[e] % U == 0, "stage write %d of %d", dst[e], R.WB());
                    if (dst[e] < 0 || dst[e] + U > R.WB()) continue;
                    for (int i = 0; i < U; ++i) {
                      CHECK(!pad[dst[e] + i], "pad byte %d written: W %d S %d l %d lane %d", dst[e] + i, t.W, t.S, l, lane);
                      st[dst[e] + i] = x[src + e * U + i];
                    }
                    ++writes;
                  }
                }
              // the windows of this iteration
              for (int g = 0; g < G; ++g) {
                const Task tk = R.task(gi0 + g, tr0, H);
                for (int r = 0; r < R.NIN(); ++r) {
                  const int row = t.S * tk.r0 - 1 + r;
                  if (row < 0 || row >= HI) {  // never read with a live filter row
                    CHECK((r == 0 && tk.top) || (r == R.NIN() - 1 && tk.bot), "row %d outside the image not masked", row);
                    ++outside;
                    continue;
                  }
                  CHECK(!(r == 0 && tk.top) && !(r == R.NIN() - 1 && tk.bot), "row %d inside the image masked", row);
                  for (int q = 0; q < R.QW(); ++q) {
                    const int wo = R.window_off(g, r, q);
                    CHECK(wo >= 0 && wo + 12 <= R.WB() && wo % 4 == 0, "window %d", wo);
                    for (int i = 0; i < 12; ++i) {
                      const int col = 4 * t.S * q - 4 + i;
                      const uint8_t want = col < 0 || col >= WI ? 0 : x[((long)(b * t.K + tk.ch) * HI + row) * WI + col];
                      CHECK(st[wo + i] == want, "window: W %d S %d n %d b %d tile %d wave %d it %d g %d row %d q %d byte %d: %d, want %d", t.W, t.S,
                            n, b, ti, wave, it, g, r, q, i, st[wo + i], want);
                    }
                    ++windows;
                  }
                }
              }
            }
          }
    }
  }
  printf("shapes %ld fetches %ld pieces %ld writes %ld windows %ld outside %ld clamped %ld bad %ld\n", shapes, fetches, pieces, writes, windows,
         outside, clamped, bad);
  return bad != 0 || shapes != 4 || !fetches || !pieces || !writes || !windows || !outside || !clamped;
}
"""


def test_every_fetch_stage_write_and_window_of_the_staged_produce():
    with tempfile.TemporaryDirectory(prefix="stream_rows.") as tmp:
        src, exe = os.path.join(tmp, "rows_main.cc"), os.path.join(tmp, "rows_main")
        with open(src, "w") as f:
            f.write(WALK)
        p = subprocess.run(["g++", "-std=c++17", "-Wall", *SANITIZE, "-I", CSRC, src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert p.returncode == 0, "stream_rows.h does not compile alone:\n" + p.stdout.decode()[-3000:]
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode()
    print(out[-3000:])
    assert r.returncode == 0, out[-3000:]
    assert "shapes 4 " in out and " bad 0" in out
