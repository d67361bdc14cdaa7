// stream_rows.h — geometry of the streaming fused dw -> pw kernel's staged produce (fused_dwpw_stream.hip, StreamShape::ROWS):
// which 16-byte piece of global memory a lane fetches, where its bytes go in the wave-private LDS stage, where a lane reads
// its row windows.  Plain constexpr C++17, no HIP: the kernel and tests/test_stream_rows_host.py (g++ alone) use the same
// functions, the way dw_plan.h is shared.
//
// A GROUP is one (channel, strip): NIN input rows of WI bytes, one contiguous span of global memory.  The span is fetched from
// its aligned-down address (HEAD junk bytes in front where rows are 56 bytes) as NPG pieces of 16 bytes.  A piece is 16 / U UNITS
// of U bytes (U = 16 for 112-byte rows, 8 for 56-byte rows): a row is UR = 7 whole units in both cases.
// A wave load fetches GPL = 1 or 2 whole groups, piece j of a group on lane j of the group's 64- or 32-lane share (the lanes
// beyond NPG fetch piece 0 again): lane -> (group, piece) is a shift and a mask, and load l differs from load 0 by a
// wave-uniform step in global memory and a constant in the stage.
// Stage of a group: NIN row slots of pitch P = WI + U: [U pad bytes][WI row bytes], one more pad behind the last slot, so column
// -1 and column WI of every row are zero bytes that are already there, and behind that a sink of U bytes.  Unit u goes to
// (u / UR) P + U + (u % UR) U, an aligned 16- or 8-byte write.  The pads are zeroed once per block and no unit ever lands on
// one; the junk units (in front of a span, behind it, those of the lanes without a piece) go to the sink.
// A lane's window of (row t, quad q) is the three aligned dwords at t P + U - 4 + 4 S q: columns 4 S q - 4 .. 4 S q + 7.
#pragma once

namespace plhip {
namespace stream_rows {

struct Task { int ch, r0; bool top, bot; };  // channel, first output row, the strip's first / last input row outside the image
struct LanePiece { int off; int dst[2]; };   // bytes from the wave's base of the iteration; stage offsets of the piece's units

struct Rows {
  int W, S, K, RS, TP;  // the instance (dw_plan.h StreamShape; W = output plane width)
  constexpr int WI() const { return S * W; }                                  // bytes of an input row
  constexpr int NIN() const { return S == 1 ? RS + 2 : 2 * RS + 1; }          // input rows of a strip
  constexpr int NS() const { return TP / W / RS; }                            // strips per tile
  constexpr int NGRP() const { return K * NS(); }                             // groups per tile
  constexpr int QW() const { return W / 4; }                                  // quads per row
  constexpr int G() const { return 64 / QW(); }                               // groups per wave and iteration
  constexpr int NIT() const { return (NGRP() + 4 * G() - 1) / (4 * G()); }    // iterations
  constexpr int U() const { return WI() % 16 == 0 ? 16 : 8; }                 // unit
  constexpr int HEAD() const { return 16 - U(); }                             // junk bytes in front of a span
  constexpr int UPP() const { return 16 / U(); }                              // units per piece
  constexpr int UR() const { return WI() / U(); }                             // units per row
  constexpr int P() const { return WI() + U(); }                              // pitch of a row slot
  constexpr int NPG() const { return (NIN() * WI() + HEAD() + 15) / 16; }     // pieces per group
  constexpr int NPGP() const { return NPG() <= 32 ? 32 : 64; }                // lanes of a load per group
  constexpr int GPL() const { return 64 / NPGP(); }                           // groups per load
  constexpr int NL() const { return (G() + GPL() - 1) / GPL(); }              // loads per iteration
  constexpr bool ragged() const { return G() % GPL() != 0; }                  // the last load has lanes without a group
  constexpr int SINK() const { return NIN() * P() + U(); }                    // a group's sink
  constexpr int GB() const { return (NIN() * P() + 2 * U() + 15) / 16 * 16; } // stage bytes of a group
  constexpr int WB() const { return G() * GB(); }                             // stage bytes of a wave
  constexpr int RD() const { return (WI() + 15) / 16 * 16; }                  // a piece of a row outside the image fetches RD bytes further in
  constexpr int src_step(int H) const { return GPL() / NS() * (S * H) * WI(); }  // load l + 1 against load l: global bytes ...
  constexpr int dst_step() const { return GPL() * GB(); }                     // ... and stage bytes
  // a piece never straddles the image's border: rows -1 | 0 and (stride 1) H - 1 | H meet on a piece boundary; the strips of a
  // wave's lanes repeat from load to load and from iteration to iteration (the per-lane offsets are loop-invariant)
  constexpr bool ok() const {
    return W % 4 == 0 && WI() % 8 == 0 && (HEAD() + WI()) % 16 == 0 && (S == 2 || (HEAD() + (NIN() - 1) * WI()) % 16 == 0) && NPG() <= 64 &&
           (4 * G()) % NS() == 0 && GPL() % NS() == 0 && UR() * U() == WI() && TP / W % RS == 0 && NGRP() >= 4 * G() && div_ok();
  }

  // group gi of a tile whose first output row is tr0 (H output rows): surplus groups of the last iteration repeat the last one,
  // strips past the image (the last tile of a 28-row plane) any valid strip
  constexpr Task task(int gi, int tr0, int H) const {
    if (gi >= NGRP()) gi = NGRP() - 1;
    const int ch = gi / NS();
    int r0 = tr0 + (gi - ch * NS()) * RS;
    if (r0 > H - RS) r0 = H - RS;
    return Task{ch, r0, r0 == 0, S == 1 && r0 + RS == H};
  }
  // global byte offset of a group's piece 0 (negative for the tensor's first strip: that piece is never fetched from there)
  constexpr int group_src(int b, const Task& t, int H) const { return ((b * K + t.ch) * (S * H) + (S * t.r0 - 1)) * WI() - HEAD(); }
  // first unit of piece j (-1: the junk in front of the span)
  constexpr int piece_unit(int j) const { return j * UPP() - (HEAD() ? 1 : 0); }
  // piece j of a group: bytes from group_src.  The pieces of a row outside the image (its filter row is zeroed, the bytes only
  // have to exist) fetch the same columns one row further in: every fetch stays inside the group's own plane
  constexpr int piece_src(int j, const Task& t) const {
    const int u0 = piece_unit(j);
    if (t.top && u0 + UPP() <= UR()) return 16 * j + RD();
    if (t.bot && u0 >= (NIN() - 1) * UR()) return 16 * j - RD();
    return 16 * j;
  }
  // stage offset (from the wave's stage) of unit u of the wave's group g
  constexpr int unit_dst(int g, int u) const {
    if (u < 0 || u >= NIN() * UR()) return g * GB() + SINK();
    return g * GB() + (u / UR()) * P() + U() + (u % UR()) * U();
  }
  constexpr int window_off(int g, int t, int q) const { return g * GB() + t * P() + U() - 4 + 4 * S * q; }
  constexpr int pad_off(int g, int k) const { return g * GB() + k * P(); }  // k = 0 .. NIN: U zero bytes each

  // what a wave fetches in an iteration whose first group is gi0 = (it 4 + wave) G: base + per-lane offset
  constexpr int wave_base(int b, int gi0, int tr0, int H) const { return group_src(b, task(gi0, tr0, H), H); }
  // x / UR for x < 64 as a multiply and a shift; the first piece that is not all row 0, the first piece of the last row
  constexpr int div_ur(int x) const { return x * (256 / UR() + 1) >> 8; }
  constexpr bool div_ok() const {
    for (int x = 0; x < 64; ++x)
      if (div_ur(x) != x / UR()) return false;
    return NIN() * UR() <= 64;
  }
  constexpr int JT() const { return (UR() + (HEAD() ? 1 : 0)) / UPP(); }
  constexpr int JB() const { return ((NIN() - 1) * UR() + (HEAD() ? 1 : 0) + UPP() - 1) / UPP(); }
  // load l of a lane: what task / group_src / piece_src / unit_dst say of its (group, piece), in selects and shifts (the
  // kernel runs it once per block); surplus = false: the caller knows that gi0 + G <= NGRP.
  // The kernel composes (fused_dwpw_stream.hip; the host test checks the composition against this function):
  //   an iteration without surplus groups, load l (not the last load where ragged()):
  //     wave_base(it) + l src_step + lane_piece(gi0 of iteration 0, lane, 0).off -> lane_piece(..).dst + l dst_step
  //   the last load where ragged(): wave_base(it) + lane_piece(gi0 of iteration 0, lane, NL - 1).off -> .dst
  //   an iteration with surplus groups: wave_base(it) + lane_piece(gi0 of it, lane, l).off, .dst as above
  constexpr LanePiece lane_piece(int gi0, int lane, int l, int tr0, int H, bool surplus = true) const {
    const int gw = lane / NPGP(), jr = lane - gw * NPGP();
    int g = l * GPL() + gw;
    const bool nogroup = g >= G(), idle = nogroup || jr >= NPG();
    g = nogroup ? 0 : g;
    const int j = idle ? 0 : jr;
    int gi = gi0 + g, g0 = gi0;
    if (surplus) {
      gi = gi < NGRP() ? gi : NGRP() - 1;
      g0 = g0 < NGRP() ? g0 : NGRP() - 1;
    }
    const int ch = gi / NS(), ch0 = g0 / NS(), last = H - RS;
    int r0 = tr0 + (gi - ch * NS()) * RS, r00 = tr0 + (g0 - ch0 * NS()) * RS;
    r0 = r0 < last ? r0 : last;
    r00 = r00 < last ? r00 : last;
    const bool top = r0 == 0, bot = S == 1 && r0 == last;
    LanePiece r = {((ch - ch0) * (S * H) + S * (r0 - r00)) * WI() + 16 * j + (top && j < JT() ? RD() : 0) - (bot && j >= JB() ? RD() : 0),
                   {0, 0}};
    const int u = piece_unit(j);
    for (int e = 0; e < UPP(); ++e) {
      const bool junk = idle || u + e < 0 || u + e >= NIN() * UR();
      r.dst[e] = g * GB() + (junk ? SINK() : (u + e + div_ur(u + e < 0 ? 0 : u + e) + 1) * U());
    }
    return r;
  }
};

}  // namespace stream_rows
}  // namespace plhip
