// Device helpers of the chunked compositing kernels (tiles.hip: tiles of 8, 16 and 32 pixels) and of the per-pixel
// lists (indices.hip): the workgroup -> (tile, pixel) mapping of the three tile sizes, the chunk's addressing block, the
// cameras' list bases, the staging of the colour rows and the halving-exchange wave reduction.
#pragma once
#include "common.h"

namespace eg {

// ts = 8: one 64-lane workgroup per tile; 16: one 256-thread workgroup per tile; 32: one per 16 x 16 quadrant
constexpr int ts_threads(int ts) { return ts == 8 ? 64 : 256; }
constexpr int ts_sub(int ts) { return ts == 32 ? 4 : 1; }  // workgroups per tile

// workgroup -> (tile, pixel of this thread); false: the workgroup's pixels all lie outside the image (uniform)
template <int TS>
__device__ __forceinline__ bool ts_pixel(int tw, int th, int width, int height, int &tile, int &i, int &j) {
  static_assert(TS == 8 || TS == 16 || TS == 32, "tile sizes 8, 16 and 32");
  constexpr int SUB = ts_sub(TS);
  const int unit = xcd_tile(blockIdx.x, tw * th * SUB);  // (the quadrants of a tile are neighbours: one XCD, mostly)
  tile = unit / SUB;
  const int q = unit % SUB, tid = threadIdx.x;
  const int ty = tile / tw, tx = tile - ty * tw;
  int i0, j0;
  if constexpr (TS == 8) {
    i0 = ty * 8; j0 = tx * 8;
    i = i0 + (tid >> 3); j = j0 + (tid & 7);
  } else {  // a 16 x 16 block of pixels: the tile (q == 0), or quadrant q of a 32-pixel tile
    i0 = ty * TS + (q >> 1) * 16; j0 = tx * TS + (q & 1) * 16;
    i = i0 + (tid >> 4); j = j0 + (tid & 15);
  }
  // (a tile's first pixel is always inside the image; a quadrant's need not be)
  return TS == 16 || (i0 < height && j0 < width);
}

struct WideArgs {
  const float *bg;    // backgrounds of the chunk: camera c's row at bg + c * cs (BG)
  float *v_depths;    // [C, N] (backward, DEPTH), accumulated
  int N;              // record stride between the cameras' blocks; EG_PACKED_STRIDE (0) = packed records (see ModeArgs)
  int colors_per_camera;
  int n_real;         // real channels of the chunk, 1 .. CH
  int cs;             // row stride (floats) of colors, v_colors and backgrounds
  int ps;             // row stride (floats) of render and v_render
  int vec;            // every colour row of the chunk starts on a 16-byte (CH = 2: 8-byte) boundary
};

// flatten_ids: the C cameras' lists one after the other, offsets [C, T+1] local to each list
__device__ __forceinline__ int wide_list_base(const int *__restrict__ offsets, int T, int c) {
  int base = 0;
  for (int k = 0; k < c; ++k) base += offsets[(size_t)k * (T + 1) + T];
  return base;
}

// Colour rows of the n Gaussians flat[first + step * r], r = 0 .. n-1, into sC[r * CH ..]: unit e = (row, 4 channels)
// is fetched by thread e % THREADS with one 16-byte load where the rows are aligned and the unit holds real channels only.
template <int CH, int THREADS>
__device__ __forceinline__ void stage_colors(float *__restrict__ sC, const float *__restrict__ colors,
                                             const int *__restrict__ flat, int first, int step, int n,
                                             const WideArgs &wa) {
  constexpr int VW = CH < 4 ? CH : 4;  // floats per unit
  constexpr int UPR = CH / VW;         // units per row
  typedef float vecw __attribute__((ext_vector_type(VW)));
  for (int e = threadIdx.x; e < n * UPR; e += THREADS) {
    const int r = e / UPR, c0 = (e % UPR) * VW;
    const float *row = colors + (size_t)flat[first + step * r] * wa.cs + c0;
    vecw v;
    if (wa.vec && c0 + VW <= wa.n_real) {
      v = *(const vecw *)row;
    } else {
#pragma unroll
      for (int k = 0; k < VW; ++k) v[k] = (c0 + k < wa.n_real) ? row[k] : 0.f;
    }
    *(vecw *)(sC + (size_t)e * VW) = v;
  }
}

// One step of the halving exchange over lane bit H, and the steps below it.
// (the step width H is a template argument: with a run-time H the indices v[k + H] are dynamic and the array leaves
// the registers)
template <int H, int K>
__device__ __forceinline__ void halving_step(float (&v)[K], int lane) {
  if constexpr (H >= 1) {
    const bool upper = (lane & H) != 0;  // this lane keeps the components whose bit H is set
#pragma unroll
    for (int k = 0; k < H; ++k) {
      const float send = upper ? v[k] : v[k + H];
      const float keep = upper ? v[k + H] : v[k];
      v[k] = keep + __shfl_xor(send, H, 64);
    }
    halving_step<H / 2, K>(v, lane);
  }
}

// Sum over the wave of each of the K values of every lane (K a power of two, 2 .. 32); returns, in every lane, the sum
// of component lane & (K - 1).  Halving exchange over the lane bits K/2, ..., 1 (K - 1 exchanges), then plain
// butterflies over the lane bits K, ..., 32.  v is clobbered.
template <int K>
__device__ __forceinline__ float lane_transpose_sum(float (&v)[K], int lane) {
  static_assert(K >= 2 && K <= 32 && (K & (K - 1)) == 0, "power of two");
  halving_step<K / 2, K>(v, lane);
  float s = v[0];
#pragma unroll
  for (int d = K; d < 64; d <<= 1) s += __shfl_xor(s, d, 64);
  return s;
}

}  // namespace eg
