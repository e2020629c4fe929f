// mi355tts host runtime — what the launch code of every precision shares: compile-time dispatch, the staged-halo table and the
// layout of a grouped launch
// (one translation unit: included once by mi355tts.hip, ahead of host_launch.h)
#pragma once

#include "tile_grid.h"

using mi355tts::int_c;

// Maps a run-time integer onto a list of compile-time values: switch_const<3, 5, 7, 11>(K, [&](auto k) { ... }) calls the lambda
// with int_c<K> (decltype(k)::value is a template argument) and returns false when v is not in the list.
template <int... Vs, class F>
static bool switch_const(int v, F&& f) {
  return ((v == Vs ? (f(int_c<Vs>{}), true) : false) || ...);
}

// LDS halo capacity of the f32 / split-bf16 conv tiles per tap count (max (K-1)*dilation the reference configs need); -1 = no tile
constexpr int conv_halo(int K) { return K == 1 ? 0 : K == 2 ? 4 : K == 3 ? 16 : K == 5 ? 28 : K == 7 ? 76 : K == 11 ? 56 : -1; }
// Does a conv fit a staged halo?  The staged tile starts at the 4-aligned column t0 - roundup(pad, 4).
constexpr bool halo_fits(int K, int dil, int pad, int halo) { return (K - 1) * dil + ((4 - pad % 4) % 4) <= halo; }

// The layout of a grouped launch: the same-geometry steps of a stage's three MRF chains as ONE 1-D grid.  Members run in tap
// order, longest-running first; member ord[i] owns workgroups [off[i], off[i + 1]) and off[3] is the grid size.  Every member's
// range is padded to a multiple of 8: the hardware deals workgroup i to XCD i % 8, and xcd_tile_lin (tile_grid.h) maps a member's
// local workgroup id onto its tiles assuming exactly that — a range that started off a multiple of 8 would put neighbouring tiles
// on different XCDs' L2s.  The padding workgroups exit at once.
struct GroupLayout {
  int ord[3];  // member indices, tap count descending
  int off[4];
  bool k1173 = false, k753 = false;  // the tap sets that have grouped kernels
};
// `tiles` in launch order
static void group_offsets(const int (&tiles)[3], int (&off)[4]) {
  off[0] = 0;
  for (int i = 0; i < 3; ++i) off[i + 1] = off[i] + ((tiles[i] + 7) & ~7);
}
// `K`, `tiles`: tap count and workgroups of each member, in the caller's order
static GroupLayout group_layout(const int (&K)[3], const int (&tiles)[3]) {
  GroupLayout l;
  for (int i = 0; i < 3; ++i) l.ord[i] = i;
  std::stable_sort(l.ord, l.ord + 3, [&](int x, int y) { return K[x] > K[y]; });
  const int k0 = K[l.ord[0]], k1 = K[l.ord[1]], k2 = K[l.ord[2]];
  l.k1173 = k0 == 11 && k1 == 7 && k2 == 3;
  l.k753 = k0 == 7 && k1 == 5 && k2 == 3;
  const int t[3] = {tiles[l.ord[0]], tiles[l.ord[1]], tiles[l.ord[2]]};
  group_offsets(t, l.off);
  return l;
}
// f(k0, k1, k2) with the layout's tap set as compile-time values; false (and no call) when the set has no grouped kernel
template <class F>
static bool switch_taps(const GroupLayout& l, F&& f) {
  if (l.k1173) f(int_c<11>{}, int_c<7>{}, int_c<3>{});
  else if (l.k753) f(int_c<7>{}, int_c<5>{}, int_c<3>{});
  return l.k1173 || l.k753;
}
