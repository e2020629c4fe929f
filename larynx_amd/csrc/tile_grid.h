// What the tile kernels share ahead of their tile functions: the XCD-aware workgroup -> tile order, the ragged-batch rule
// (row_tiles; row_gx and member_tile apply it to a member of a grouped launch), the member dispatch of a grouped launch
// (group_member, pick3), a batch row's length and the accumulator row map of the 32x32 MFMA blocks.  Included by conv_mfma.h,
// and so by every tile.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace mi355tts {

// a compile-time integer as a value, for generic lambdas (host_group.h: switch_const, switch_taps)
template <int V>
using int_c = std::integral_constant<int, V>;

constexpr int max3(int a, int b, int c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

// Length of batch row b: per-row counts on the device times a fixed factor, or one value for the whole launch when there is
// no array (batch 1).  B: the kernels index with an int or with blockIdx.z itself.
template <class B>
__device__ __forceinline__ int tile_len(const int* len, int mul, int len_const, B b) { return len ? len[b] * mul : len_const; }

// C/D layout of the 32x32 MFMAs: accumulator register r of a lane holds column lane & 31 of block row
// acc_row(r) + 4 * (lane >> 5).  Registers r and r + 8 are rows i and i + 16; 4g .. 4g + 3 are four consecutive rows.
__device__ __forceinline__ constexpr int acc_row(int r) { return (r & 3) + 8 * (r >> 2); }

// XCD-aware tile order.  The dispatcher deals workgroup `lin` to XCD `lin % 8`, each XCD
// with its own L2.  Tiles that share input (the m-tiles of one time tile, and
// neighbouring time tiles through the halo) should meet in ONE L2, so the linear id is
// re-dealt: XCD x gets a contiguous run of tiles, m-tile fastest.  Bijective for any n
// (MI355X_MICROARCH.md, T1); a wrong placement guess costs speed, never correctness.
//
// `rows_major` != 0 flips the order inside the run: XCD x then owns a contiguous range of ROW tiles (with all
// their time tiles), i.e. 1/8 of the weights — for launches whose packed weights do not fit one 4 MB L2 while
// their input does (the stage-0 upsampler of HiFi-GAN 'high': 8.4 MB of weights, 1.3 MB of input; with time
// dealt across the XCDs every XCD streamed all 8.4 MB once per time tile: 86 MB fetched per launch).
__device__ __forceinline__ void xcd_tile_lin(int lin, int gx, int gy, int& tx, int& ty, int rows_major = 0) {
  const int n = gx * gy;
  const int xcd = lin & 7, slot = lin >> 3;
  const int q = n >> 3, r = n & 7;
  const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
  if (rows_major) {
    tx = id % gx;
    ty = id / gx;
  } else {
    ty = id % gy;
    tx = id / gy;
  }
}
__device__ __forceinline__ void xcd_tile(int gx, int gy, int& tx, int& ty, int rows_major = 0) {
  xcd_tile_lin(blockIdx.x + blockIdx.y * gx, gx, gy, tx, ty, rows_major);
}

// Ragged batches (gridDim.z > 1 rows of different lengths): the grid is sized for the longest row, and dealing
// contiguous runs of the GRID's tiles to the XCDs would hand a short row's few real tiles to XCD 0 (and 1) alone —
// over a batch of 8 rows with lengths 0.14 ... 1.0 of the longest, XCD 0 gets 8 shares of work and XCD 7 one
// (measured on BASELINE config 4: the 32-channel fused pair launches ran at 0.24 of peak against 0.59 at batch 1).
// So a row deals only ITS OWN tiles: the first gx_row * gy workgroups of the row's grid slice take them (spread
// evenly over the XCDs by the dispatcher's round-robin), the rest exit.
__device__ __forceinline__ int row_tiles(int n_len, int tile) { return (n_len + tile - 1) / tile; }

// The ragged rule, in the one place every tile kernel takes it from.  Time tiles of this workgroup's batch row: the row's own
// (`tile` columns each) when the launch has rows of different lengths, else the count the grid was sized with.  `row_len` is a
// callable (forced inline, like every callback here), so a launch of one row never reads the length array.
template <class L>
__device__ __forceinline__ int row_gx(int gx_grid, int tile, L&& row_len) { return gridDim.z > 1 ? row_tiles(row_len(), tile) : gx_grid; }

// Workgroup l of a member of a grouped launch (below; a gx x gy tile grid in a range padded to a multiple of 8): false past the
// row's own tiles, else its tile in the XCD-aware order.  The fused pairs have time tiles only: gy = 1, ty unused.
template <class L>
__device__ __forceinline__ bool member_tile(int l, int gx_grid, int gy, int tile, L&& row_len, int& tx, int& ty) {
  const int gx = row_gx(gx_grid, tile, row_len);
  if (l >= gx * gy) return false;
  xcd_tile_lin(l, gx, gy, tx, ty);
  return true;
}

// Grouped launches (conv_mfma.h, conv_group_kernel): the three MRF chains' same-geometry tiles in one 1-D grid, member 0's
// first.  What differs between the members is compile-time (taps, halo), so the member index reaches the callback as an
// int_c: f(int_c<m>{}, l) with l the workgroup's index inside member m; pick3<m, K0, K1, K2> is then that member's value.
// Callbacks are lambdas marked __attribute__((always_inline)): a tile body behind a real call would lose its registers.
// In use by pair_group_kernel (resblock_pair.h), whose code it leaves byte-identical.  The other seven grouped kernels and
// the kernels of one conv per launch keep the rule and the ladder written out: the helper form moves their code generation,
// and their launch times left the written-out form's own spread when measured (profiles/NOTES.md, tools/isa_diff.py).
template <int M, int V0, int V1, int V2>
constexpr int pick3 = M == 0 ? V0 : M == 1 ? V1 : V2;

// the plain longest-first order: workgroups off[m] .. off[m + 1] are member m's
template <class F>
__device__ __forceinline__ void group_member(const int (&off)[4], int lin, F&& f) {
  if (lin < off[1]) f(int_c<0>{}, lin);
  else if (lin < off[2]) f(int_c<1>{}, lin - off[1]);
  else f(int_c<2>{}, lin - off[2]);
}

}  // namespace mi355tts
