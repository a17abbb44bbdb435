// Bilateral grid (edgegaussians_amd/bilagrid.py): the trilinear slice of a per-image lattice of 3x4 affine colour
// transforms applied to a render, its backward, and the total-variation regulariser of all grids.
//
//   grids [N, 12, L, Hg, Wg];  image b uses grid g = grid_idx[b] (or b).  Per sample (r, g, b; x, y):
//   gray = (0.299f r + 0.587f g) + 0.114f b;   u = clamp(x (Wg - 1), 0, Wg - 1), v = clamp(y (Hg - 1), 0, Hg - 1),
//   w = clamp(gray (L - 1), 0, L - 1);  per axis of size n: i0 = min(floor(u), n - 2) (0 when n == 1), t = u - i0,
//   i1 = min(i0 + 1, n - 1).  A[c, k] = the trilinear blend of grids[g, 4 c + k] at (w, v, u), evaluated as nested
//   lerps a + t (b - a): four along x, two along y, one along z -- 9 roundings on the longest chain, and a grid that
//   is constant over its cells gives that constant EXACTLY (b - a = 0), so identity grids return rgb bit for bit.
//   out_c = ((A[c,0] r + A[c,1] g) + A[c,2] b) + A[c,3].
//   Backward for a cotangent v of out:
//   v_rgb_k = sum_c v_c A[c,k] + gw_k (L - 1) gate sum_c v_c sum_k' (r, g, b, 1)_k' dA[c,k'],  dA = the xy blend at
//   l1 minus the xy blend at l0, gate = 0 < gray (L - 1) < L - 1 (unclamped; torch's border rule), a select;
//   v_grids[g, 4 c + k, corner] += w_corner v_c (r, g, b, 1)_k,  w_corner = (wz wy) wx with weights (1 - t, t).
//
// Kernels.  Forward and v_rgb are pure maps, one lane per sample (v_rgb: the same bits every run), each a sample of
// fwd_sample / vrgb_sample: 96 grid words per sample.  While one grid, 48 L Hg Wg bytes, fits EG_BILAGRID_LDS_BUDGET
// (slice_map_lds_kernel) up to 256 persistent workgroups of 1024 lanes each copy their image's grid into LDS once and read
// the corners from there (the 32 KiB L1 is smaller than the grid, so from global memory every corner is an L2 access);
// larger grids (slice_map_kernel) read them where they lie.  The arithmetic is one code path, so both give the same bits.
// slice_vgrid_kernel: the scatter.  Plain global float atomics would add 96 floats = 384 B per sample against a
// chip-wide atomic rate of about 1.3 TB/s: 0.6 ms at 1200 x 1600, an order of magnitude over everything else here.  So
// while 48 L Hg Wg bytes fit EG_BILAGRID_LDS_BUDGET a workgroup of 1024 lanes keeps a private copy of its image's grid
// gradient in LDS, adds the samples of its block of pixels there (lane t owns `run` consecutive samples, so the lanes
// of a wave are `run` samples apart and mostly in different cells), and flushes the non-zero words with one global
// float atomic each, 256 contiguous bytes per wave-instruction.  Larger grids: slice_vgrid_global_kernel, one lane per
// sample, where a wave whose 64 samples share their base cell adds them up with the DPP tree and issues one atomic
// per word, and any other wave one per lane.  Both forms add floats in arrival order: v_grids is NOT bit-reproducible.
// Measured (profiles/bilagrid_timing.txt): the LDS scatter takes 1.06 ms at 1200 x 1600 -- 3.5 cycles per
// ds_add_f32 lane-operation per CU, no better than the global atomics it was sized against; it is the call's whole cost.
// tv_fwd_kernel / tv_finalize_kernel: the reduction of losses.hip (a lane's 4 cells x 3 axes in order, block_sum_f,
// one partial per workgroup, slab_sum_f by one wave); tv_bwd_kernel: one gather pass, each cell from its <= 6
// neighbours.  No atomics in either: the same bits every run.  Contraction is off: every operation rounds as written
// (tests/bilagrid_util.py counts them).
#include "common.h"

using namespace eg;

namespace {

constexpr int kThreads = 256;          // lanes of a workgroup of the TV kernels and of the kernels for grids above the budget
constexpr int kMapThreads = 1024;      // lanes of a persistent workgroup of the forward and v_rgb kernels (bilagrid.py: MAP_THREADS)
constexpr int kScatterThreads = 1024;  // lanes of a workgroup of the LDS scatter (bilagrid.py: SCATTER_THREADS)
constexpr int kTvQuad = 4;             // consecutive cells of a lane of the TV forward
constexpr int kTvPerWG = kThreads * kTvQuad;  // (bilagrid.py: TV_WG_ELEMS)
constexpr int kFinLanes = 64;
static_assert(kFinLanes == kWave, "slab_sum_f is one wave");
constexpr int kPersistentWGs = 256;  // persistent workgroups of the LDS kernels: one per CU

struct Strides {
  int64_t b, h, w, c;
};
struct Problem {
  const float *grids;
  const void *grid_idx;  // NULL: image b uses grid b
  int idx64;
  int N, L, Hg, Wg;
  uint32_t H, W;         // samples of an image: H W
  uint32_t n;            // B H W < 2^31
};
struct Sample {
  float p[3];            // r g b
  int i0, j0, l0, i1, j1, l1;
  float tx, ty, tz;
  bool gate;
};

__device__ __forceinline__ int grid_of(const Problem &P, uint32_t b) {
  if (!P.grid_idx) return (int)b;
  const long long g = P.idx64 ? static_cast<const long long *>(P.grid_idx)[b] : static_cast<const int *>(P.grid_idx)[b];
  return (int)(g < 0 ? 0 : (g >= P.N ? P.N - 1 : g));  // (range-checked by the caller; clamped so that no index leaves the grids)
}

// cell and fraction of a coordinate on an axis of n cells; NaN lands in cell 0
__device__ __forceinline__ void axis(float u, int n, int &i0, int &i1, float &t) {
  const float top = (float)(n - 1);
  u = fminf(fmaxf(u, 0.f), top);
  i0 = max(min((int)floorf(u), n - 2), 0);
  i1 = min(i0 + 1, n - 1);
  t = u - (float)i0;
}

__device__ __forceinline__ void load3(const float *p, int64_t sc, float (&o)[3]) {
  o[0] = p[0], o[1] = p[sc], o[2] = p[2 * sc];
}

// sample s (< P.n) of the logical [B, H, W] problem
__device__ __forceinline__ Sample locate(const Problem &P, const float *__restrict__ rgb, const Strides &sr,
                                         const float *__restrict__ xy, const Strides &sx, uint32_t s, uint32_t &b) {
#pragma clang fp contract(off)
  const uint32_t row = s / P.W, w = s - row * P.W;
  b = row / P.H;
  const uint32_t h = row - b * P.H;
  Sample q;
  load3(rgb + (b * sr.b + h * sr.h + w * sr.w), sr.c, q.p);
  const float *c = xy + (b * sx.b + h * sx.h + w * sx.w);
  const float x = c[0], y = c[sx.c];
  const float gray = (0.299f * q.p[0] + 0.587f * q.p[1]) + 0.114f * q.p[2];
  const float top = (float)(P.L - 1), wraw = gray * top;
  q.gate = wraw > 0.f && wraw < top;
  axis(x * (float)(P.Wg - 1), P.Wg, q.i0, q.i1, q.tx);
  axis(y * (float)(P.Hg - 1), P.Hg, q.j0, q.j1, q.ty);
  axis(wraw, P.L, q.l0, q.l1, q.tz);
  return q;
}

__device__ __forceinline__ float lerp(float a, float b, float t) {
#pragma clang fp contract(off)
  return a + t * (b - a);
}

// image b's grid [12, L, Hg, Wg] in global memory
__device__ __forceinline__ const float *grid_at(const Problem &P, uint32_t b) {
  return P.grids + (size_t)grid_of(P, b) * 12 * P.L * P.Hg * P.Wg;
}

// the xy blends of channel ch of `grid` (global memory or the workgroup's LDS copy) at l0 and l1
__device__ __forceinline__ void blend_xy(const Problem &P, const Sample &q, const float *grid, int ch, float &at0,
                                         float &at1) {
  const float *g = grid + ch * (P.L * P.Hg * P.Wg);
  const int r00 = (q.l0 * P.Hg + q.j0) * P.Wg, r01 = (q.l0 * P.Hg + q.j1) * P.Wg;
  const int r10 = (q.l1 * P.Hg + q.j0) * P.Wg, r11 = (q.l1 * P.Hg + q.j1) * P.Wg;
  at0 = lerp(lerp(g[r00 + q.i0], g[r00 + q.i1], q.tx), lerp(g[r01 + q.i0], g[r01 + q.i1], q.tx), q.ty);
  at1 = lerp(lerp(g[r10 + q.i0], g[r10 + q.i1], q.tx), lerp(g[r11 + q.i0], g[r11 + q.i1], q.tx), q.ty);
}

__device__ __forceinline__ void fwd_sample(const Problem &P, const Sample &q, const float *grid, float *__restrict__ dst) {
#pragma clang fp contract(off)
  float o[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float A[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float a0, a1;
      blend_xy(P, q, grid, 4 * c + k, a0, a1);
      A[k] = lerp(a0, a1, q.tz);
    }
    o[c] = ((A[0] * q.p[0] + A[1] * q.p[1]) + A[2] * q.p[2]) + A[3];
  }
  dst[0] = o[0], dst[1] = o[1], dst[2] = o[2];
}

__device__ __forceinline__ void vrgb_sample(const Problem &P, const Sample &q, const float *grid,
                                            const float *__restrict__ vs, float *__restrict__ dst) {
#pragma clang fp contract(off)
  float direct[3] = {0.f, 0.f, 0.f}, D = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float vc = vs[c];
    float A[4], dA[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float a0, a1;
      blend_xy(P, q, grid, 4 * c + k, a0, a1);
      A[k] = lerp(a0, a1, q.tz);
      dA[k] = a1 - a0;
    }
    const float qc = ((dA[0] * q.p[0] + dA[1] * q.p[1]) + dA[2] * q.p[2]) + dA[3];
    if (c == 0) {
      D = vc * qc;
#pragma unroll
      for (int k = 0; k < 3; ++k) direct[k] = vc * A[k];
    } else {
      D = D + vc * qc;
#pragma unroll
      for (int k = 0; k < 3; ++k) direct[k] = direct[k] + vc * A[k];
    }
  }
  const float top = (float)(P.L - 1);
  const float gw[3] = {0.299f, 0.587f, 0.114f};
#pragma unroll
  for (int k = 0; k < 3; ++k) dst[k] = q.gate ? direct[k] + (gw[k] * top) * D : direct[k];  // (a select: no 0 * inf)
}

// Grids above the LDS budget: one lane per sample, the grid read where it lies.  VRGB: v_rgb from v, else out.
template <bool VRGB>
__global__ void __launch_bounds__(kThreads)
slice_map_kernel(Problem P, const float *__restrict__ rgb, Strides sr, const float *__restrict__ xy, Strides sx,
                 const float *__restrict__ v, float *__restrict__ dst) {
  const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
  if (s >= P.n) return;
  uint32_t b;
  const Sample q = locate(P, rgb, sr, xy, sx, s, b);
  if (VRGB) vrgb_sample(P, q, grid_at(P, b), v + (size_t)s * 3, dst + (size_t)s * 3);
  else fwd_sample(P, q, grid_at(P, b), dst + (size_t)s * 3);
}

// Grids inside the budget: persistent workgroups, `blocks` per image (workgroup blockIdx.x belongs to image
// blockIdx.x / blocks), each with its image's grid in LDS; the workgroups of an image deal its samples kMapThreads at a
// time, lane = sample.  The arithmetic is fwd_sample / vrgb_sample either way.
template <bool VRGB>
__global__ void __launch_bounds__(kMapThreads)
slice_map_lds_kernel(Problem P, const float *__restrict__ rgb, Strides sr, const float *__restrict__ xy, Strides sx,
                     const float *__restrict__ v, uint32_t blocks, float *__restrict__ dst) {
  extern __shared__ __attribute__((aligned(16))) float s_grid[];
  const uint32_t b = blockIdx.x / blocks, block = blockIdx.x - b * blocks, per_image = P.H * P.W;
  const int words = 12 * P.L * P.Hg * P.Wg;
  const float *src = grid_at(P, b);
  for (int i = threadIdx.x; i < words; i += kMapThreads) s_grid[i] = src[i];
  __syncthreads();
  for (uint64_t in_image = (uint64_t)block * kMapThreads + threadIdx.x; in_image < per_image;
       in_image += (uint64_t)blocks * kMapThreads) {
    const uint32_t s = b * per_image + (uint32_t)in_image;
    uint32_t b_;
    const Sample q = locate(P, rgb, sr, xy, sx, s, b_);
    if (VRGB) vrgb_sample(P, q, s_grid, v + (size_t)s * 3, dst + (size_t)s * 3);
    else fwd_sample(P, q, s_grid, dst + (size_t)s * 3);
  }
}

// the 8 corner weights (wz wy) wx and the cells they go to
__device__ __forceinline__ void corners(const Problem &P, const Sample &q, float (&w)[8], int (&cell)[8]) {
#pragma clang fp contract(off)
  const float wx[2] = {1.f - q.tx, q.tx}, wy[2] = {1.f - q.ty, q.ty}, wz[2] = {1.f - q.tz, q.tz};
  const int ii[2] = {q.i0, q.i1}, jj[2] = {q.j0, q.j1}, ll[2] = {q.l0, q.l1};
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    const int z = a >> 2, y = (a >> 1) & 1, x = a & 1;
    w[a] = (wz[z] * wy[y]) * wx[x];
    cell[a] = (ll[z] * P.Hg + jj[y]) * P.Wg + ii[x];
  }
}

// Persistent workgroups, `blocks` per image: workgroup blockIdx.x takes block blockIdx.x % blocks, kScatterThreads *
// run samples, of image blockIdx.x / blocks; acc (LDS) is its copy of the image's grid gradient [12, cells].
__global__ void __launch_bounds__(kScatterThreads)
slice_vgrid_kernel(Problem P, const float *__restrict__ rgb, Strides sr, const float *__restrict__ xy, Strides sx,
                   const float *__restrict__ v, uint32_t blocks, uint32_t run, float *__restrict__ v_grids) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float acc[];
  const int cells = P.L * P.Hg * P.Wg, words = 12 * cells;
  for (int i = threadIdx.x; i < words; i += kScatterThreads) acc[i] = 0.f;
  __syncthreads();
  const uint32_t per_image = P.H * P.W, b = blockIdx.x / blocks, block = blockIdx.x - b * blocks;
  const uint64_t first = ((uint64_t)block * kScatterThreads + threadIdx.x) * run;
  for (uint32_t k = 0; k < run; ++k) {
    const uint64_t in_image = first + k;
    if (in_image >= per_image) break;
    const uint32_t s = b * per_image + (uint32_t)in_image;
    uint32_t b_;
    const Sample q = locate(P, rgb, sr, xy, sx, s, b_);
    float w[8];
    int cell[8];
    corners(P, q, w, cell);
    const float *vs = v + (size_t)s * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float vc = vs[c];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const float vp = kk < 3 ? vc * q.p[kk] : vc;
        float *dst = acc + (4 * c + kk) * cells;
#pragma unroll
        for (int a = 0; a < 8; ++a) atomicAdd(dst + cell[a], w[a] * vp);
      }
    }
  }
  __syncthreads();
  float *g = v_grids + (size_t)grid_of(P, b) * words;
  for (int i = threadIdx.x; i < words; i += kScatterThreads) {
    const float x = acc[i];
    if (x != 0.f) atomicAdd(g + i, x);
  }
}

// Grids above the LDS budget: one lane per sample, every lane of a wave active to the end (lanes from n on carry
// weights of zero on sample n - 1's cells).
__global__ void __launch_bounds__(kThreads)
slice_vgrid_global_kernel(Problem P, const float *__restrict__ rgb, Strides sr, const float *__restrict__ xy, Strides sx,
                          const float *__restrict__ v, float *__restrict__ v_grids) {
#pragma clang fp contract(off)
  const uint32_t s_raw = blockIdx.x * kThreads + threadIdx.x;
  const bool live = s_raw < P.n;
  const uint32_t s = live ? s_raw : P.n - 1;
  uint32_t b;
  const Sample q = locate(P, rgb, sr, xy, sx, s, b);
  float w[8];
  int cell[8];
  corners(P, q, w, cell);
  const int cells = P.L * P.Hg * P.Wg;
  const int g = grid_of(P, b);
  float *base = v_grids + (size_t)g * 12 * cells;
  const float *vs = v + (size_t)s * 3;
  // one base cell for the whole wave: the 8 corner cells are shared too
  const int key = ((g * P.L + q.l0) * P.Hg + q.j0) * P.Wg + q.i0;
  const bool shared = __all(key == __builtin_amdgcn_readfirstlane(key));
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float vc = live ? vs[c] : 0.f;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const float vp = kk < 3 ? vc * q.p[kk] : vc;
      float *dst = base + (size_t)(4 * c + kk) * cells;
#pragma unroll
      for (int a = 0; a < 8; ++a) {
        const float term = live ? w[a] * vp : 0.f;
        if (shared) {
          const float total = wave_sum_dpp_f(term);
          if ((threadIdx.x & 63) == 63 && total != 0.f) atomicAdd(dst + cell[a], total);
        } else if (term != 0.f) {
          atomicAdd(dst + cell[a], term);
        }
      }
    }
  }
}

struct TvShape {
  int L, Hg, Wg;
  uint32_t n;                // N 12 L Hg Wg < 2^31
  float inv_l, inv_h, inv_w; // 1 / count_a, 0 for an axis of size 1
};

// cell e -> (l, j, i); the (n, channel) plane does not matter
__device__ __forceinline__ void tv_index(uint32_t e, const TvShape &s, int &l, int &j, int &i) {
  const uint32_t row = e / s.Wg, plane = row / s.Hg;
  i = e - row * s.Wg, j = row - plane * s.Hg, l = plane % s.L;
}

__global__ void __launch_bounds__(kThreads)
tv_fwd_kernel(const float *__restrict__ x, TvShape s, float *__restrict__ slab) {
#pragma clang fp contract(off)
  __shared__ float wave_f[kThreads / kWave];
  const uint32_t e0 = (blockIdx.x * kThreads + threadIdx.x) * kTvQuad;
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < kTvQuad; ++k) {
    const uint32_t e = e0 + k;
    float tl = 0.f, th = 0.f, tw = 0.f;
    if (e < s.n) {
      int l, j, i;
      tv_index(e, s, l, j, i);
      const float c = x[e];
      if (l + 1 < s.L) { const float d = x[e + s.Hg * s.Wg] - c; tl = (d * d) * s.inv_l; }
      if (j + 1 < s.Hg) { const float d = x[e + s.Wg] - c; th = (d * d) * s.inv_h; }
      if (i + 1 < s.Wg) { const float d = x[e + 1] - c; tw = (d * d) * s.inv_w; }
    }
    acc = ((acc + tl) + th) + tw;
  }
  const float total = block_sum_f<kThreads>(acc, wave_f);
  if (threadIdx.x == 0) slab[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kFinLanes)
tv_finalize_kernel(const float *__restrict__ slab, int G, float *__restrict__ out) {
  const float sum = slab_sum_f(slab, G, 1);
  if (threadIdx.x == kFinLanes - 1) out[0] = sum;
}

__global__ void __launch_bounds__(kThreads)
tv_bwd_kernel(const float *__restrict__ x, TvShape s, const float *__restrict__ v, float *__restrict__ g) {
#pragma clang fp contract(off)
  const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= s.n) return;
  int l, j, i;
  tv_index(e, s, l, j, i);
  const float c = x[e];
  const int sl = s.Hg * s.Wg, sh = s.Wg;
  const float dl = (l > 0 ? c - x[e - sl] : 0.f) - (l + 1 < s.L ? x[e + sl] - c : 0.f);
  const float dh = (j > 0 ? c - x[e - sh] : 0.f) - (j + 1 < s.Hg ? x[e + sh] - c : 0.f);
  const float dw = (i > 0 ? c - x[e - 1] : 0.f) - (i + 1 < s.Wg ? x[e + 1] - c : 0.f);
  const float sum = (dl * (2.f * s.inv_l) + dh * (2.f * s.inv_h)) + dw * (2.f * s.inv_w);
  g[e] = v[0] * sum;
}

inline Strides strides_of(const int64_t *st) { return {st[0], st[1], st[2], st[3]}; }

inline float inv_count(int64_t planes, int n_axis, int64_t others) {
  return n_axis > 1 ? 1.0f / (float)((double)planes * (n_axis - 1) * others) : 0.f;
}

#define EG_BILAGRID_CHECK_GRIDS()                                                                              \
  do {                                                                                                         \
    EG_REQUIRE(N >= 1 && L >= 1 && Hg >= 1 && Wg >= 1, "bad grid sizes (N, L, Hg, Wg >= 1)");                  \
    EG_REQUIRE((int64_t)N * 12 * L * Hg * Wg < ((int64_t)1 << 31), "N * 12 * L * Hg * Wg must be below 2^31"); \
    EG_REQUIRE(grids, "null grids");                                                                           \
  } while (0)

#define EG_BILAGRID_CHECK_SLICE()                                                                      \
  do {                                                                                                 \
    EG_BILAGRID_CHECK_GRIDS();                                                                         \
    EG_REQUIRE(B >= 1 && H >= 1 && W >= 1, "bad sizes (B, H, W >= 1)");                                \
    EG_REQUIRE((int64_t)B * H * W < ((int64_t)1 << 31), "B * H * W must be below 2^31");               \
    EG_REQUIRE(rgb && xy, "null rgb / xy");                                                            \
    EG_REQUIRE(grid_idx || B == N, "grid_idx: NULL needs B == N");                                     \
    EG_REQUIRE(idx_is_int64 == 0 || idx_is_int64 == 1, "idx_is_int64 must be 0 or 1");                 \
    EG_REQUIRE(strides_rgb && strides_xy, "null strides_rgb / strides_xy");                            \
    for (int i = 0; i < 4; ++i) EG_REQUIRE(strides_rgb[i] >= 0 && strides_xy[i] >= 0, "negative stride"); \
    EG_REQUIRE(max_workgroups >= 0, "max_workgroups must be >= 0 (0: one per CU)");                     \
  } while (0)

inline Problem problem_of(const float *grids, const void *grid_idx, int idx64, int N, int L, int Hg, int Wg, int B, int H,
                          int W) {
  return {grids, grid_idx, idx64, N, L, Hg, Wg, (uint32_t)H, (uint32_t)W, (uint32_t)((int64_t)B * H * W)};
}

// an LDS kernel may take the whole budget as dynamic LDS: above 64 KiB that has to be asked for, per kernel and per
// device, so it is asked before every launch (a host-side call without a device round trip)
inline bool allow_lds_budget(const void *kernel) {
  return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, EG_BILAGRID_LDS_BUDGET) == hipSuccess;
}

// workgroups per image of a persistent LDS kernel: max_workgroups (0: kPersistentWGs, one per CU) over the B images,
// at least one per image, never more than one per `threads` samples
inline int64_t persistent_blocks(int B, int64_t per_image, int threads, int max_workgroups) {
  const int64_t all = max_workgroups > 0 ? max_workgroups : kPersistentWGs;
  const int64_t most = (per_image + threads - 1) / threads;
  const int64_t blocks = (all + B - 1) / B;
  return blocks < 1 ? 1 : (blocks > most ? most : blocks);
}

template <bool VRGB>
bool launch_map(const Problem &P, int B, const float *rgb, const Strides &sr, const float *xy, const Strides &sx,
                const float *v, int max_workgroups, float *dst, hipStream_t st) {
  const int64_t lds = (int64_t)48 * P.L * P.Hg * P.Wg;
  if (lds <= EG_BILAGRID_LDS_BUDGET) {
    if (!allow_lds_budget((const void *)slice_map_lds_kernel<VRGB>)) return false;
    const int64_t blocks = persistent_blocks(B, (int64_t)P.H * P.W, kMapThreads, max_workgroups);  // (B blocks <= B H W < 2^31)
    slice_map_lds_kernel<VRGB><<<(unsigned)(blocks * B), kMapThreads, (size_t)lds, st>>>(P, rgb, sr, xy, sx, v,
                                                                                        (uint32_t)blocks, dst);
  } else {
    slice_map_kernel<VRGB><<<cdiv(P.n, kThreads), kThreads, 0, st>>>(P, rgb, sr, xy, sx, v, dst);
  }
  return true;
}

#define EG_BILAGRID_LDS_REFUSED()                                                                     \
  do {                                                                                                \
    set_error("%s: the device refused %d bytes of dynamic LDS", __func__, EG_BILAGRID_LDS_BUDGET);    \
    return EG_ERR_LAUNCH;                                                                             \
  } while (0)

}  // namespace

extern "C" int eg_bilagrid_slice_fwd(const float *grids, int32_t N, int32_t L, int32_t Hg, int32_t Wg, const float *rgb,
                                     const float *xy, const void *grid_idx, int32_t idx_is_int64, int32_t B, int32_t H,
                                     int32_t W, const int64_t *strides_rgb, const int64_t *strides_xy,
                                     int32_t max_workgroups, float *out, eg_stream_t stream) {
  EG_BILAGRID_CHECK_SLICE();
  EG_REQUIRE(out, "null out");
  const Problem P = problem_of(grids, grid_idx, idx_is_int64, N, L, Hg, Wg, B, H, W);
  if (!launch_map<false>(P, B, rgb, strides_of(strides_rgb), xy, strides_of(strides_xy), nullptr, max_workgroups, out,
                         as_stream(stream)))
    EG_BILAGRID_LDS_REFUSED();
  return check_launch("bilagrid_slice_fwd");
}

extern "C" int eg_bilagrid_slice_bwd(const float *grids, int32_t N, int32_t L, int32_t Hg, int32_t Wg, const float *rgb,
                                     const float *xy, const void *grid_idx, int32_t idx_is_int64, int32_t B, int32_t H,
                                     int32_t W, const int64_t *strides_rgb, const int64_t *strides_xy,
                                     int32_t max_workgroups, const float *v, float *v_rgb, float *v_grids,
                                     eg_stream_t stream) {
  EG_BILAGRID_CHECK_SLICE();
  EG_REQUIRE(v, "null v");
  EG_REQUIRE(v_rgb || v_grids, "v_rgb and v_grids both null: nothing to do");
  const Problem P = problem_of(grids, grid_idx, idx_is_int64, N, L, Hg, Wg, B, H, W);
  const Strides sr = strides_of(strides_rgb), sx = strides_of(strides_xy);
  hipStream_t st = as_stream(stream);
  if (v_rgb && !launch_map<true>(P, B, rgb, sr, xy, sx, v, max_workgroups, v_rgb, st)) EG_BILAGRID_LDS_REFUSED();
  if (v_grids) {
    const int64_t lds = (int64_t)48 * L * Hg * Wg;
    if (lds <= EG_BILAGRID_LDS_BUDGET) {
      if (!allow_lds_budget((const void *)slice_vgrid_kernel)) EG_BILAGRID_LDS_REFUSED();
      const int64_t per_image = (int64_t)H * W;
      int64_t blocks = persistent_blocks(B, per_image, kScatterThreads, max_workgroups);
      const int64_t run = (per_image + blocks * kScatterThreads - 1) / (blocks * kScatterThreads);
      blocks = (per_image + run * kScatterThreads - 1) / (run * kScatterThreads);
      slice_vgrid_kernel<<<(unsigned)(blocks * B), kScatterThreads, (size_t)lds, st>>>(P, rgb, sr, xy, sx, v, (uint32_t)blocks,
                                                                                      (uint32_t)run, v_grids);
    } else {
      slice_vgrid_global_kernel<<<cdiv(P.n, kThreads), kThreads, 0, st>>>(P, rgb, sr, xy, sx, v, v_grids);
    }
  }
  return check_launch("bilagrid_slice_bwd");
}

extern "C" int eg_bilagrid_tv_fwd(const float *grids, int32_t N, int32_t L, int32_t Hg, int32_t Wg, float *slab,
                                  int64_t slab_len, float *out, eg_stream_t stream) {
  EG_BILAGRID_CHECK_GRIDS();
  const int64_t n = (int64_t)N * 12 * L * Hg * Wg, planes = (int64_t)N * 12;
  const int G = cdiv(n, kTvPerWG);
  EG_REQUIRE(slab && out, "null slab / out");
  EG_REQUIRE(slab_len >= G, "slab too small (ceil(N 12 L Hg Wg / 1024) floats)");
  const TvShape s = {L, Hg, Wg, (uint32_t)n, inv_count(planes, L, (int64_t)Hg * Wg), inv_count(planes, Hg, (int64_t)L * Wg),
                     inv_count(planes, Wg, (int64_t)L * Hg)};
  hipStream_t st = as_stream(stream);
  tv_fwd_kernel<<<G, kThreads, 0, st>>>(grids, s, slab);
  tv_finalize_kernel<<<1, kFinLanes, 0, st>>>(slab, G, out);
  return check_launch("bilagrid_tv_fwd");
}

extern "C" int eg_bilagrid_tv_bwd(const float *grids, int32_t N, int32_t L, int32_t Hg, int32_t Wg, const float *v,
                                  float *v_grids, eg_stream_t stream) {
  EG_BILAGRID_CHECK_GRIDS();
  EG_REQUIRE(v && v_grids, "null v / v_grids");
  const int64_t n = (int64_t)N * 12 * L * Hg * Wg, planes = (int64_t)N * 12;
  const TvShape s = {L, Hg, Wg, (uint32_t)n, inv_count(planes, L, (int64_t)Hg * Wg), inv_count(planes, Hg, (int64_t)L * Wg),
                     inv_count(planes, Wg, (int64_t)L * Hg)};
  tv_bwd_kernel<<<cdiv(n, kThreads), kThreads, 0, as_stream(stream)>>>(grids, s, v, v_grids);
  return check_launch("bilagrid_tv_bwd");
}
