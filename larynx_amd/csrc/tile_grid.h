// What the tile kernels share ahead of their tile functions: the XCD-aware workgroup -> tile order, the ragged-batch rule,
// a batch row's length and the accumulator row map of the 32x32 MFMA blocks.  Included by conv_mfma.h, and so by every tile.
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

}  // namespace mi355tts
