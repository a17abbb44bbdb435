// Fused SSIM (the `fused_ssim` operation of 3DGS trainers) and its backward: two kernels, one launch each.
//
//   G*x      the 11-tap Gaussian (sigma 1.5) along W, then along H, zero padding of 5, per (b, c) plane
//   m1 = G*x1, m2 = G*x2, e11 = G*x1^2, e22 = G*x2^2, e12 = G*(x1 x2);  s1 = e11 - m1^2, s2 = e22 - m2^2, s12 = e12 - m1 m2
//   A1 = 2 m1 m2 + C1, A2 = 2 s12 + C2, B1 = m1^2 + m2^2 + C1, B2 = s1 + s2 + C2;  S = A1 A2 / (B1 B2)
//   backward for a cotangent v of S:  v_x1 = G*(v d_m1) + 2 x1 G*(v d_s1) + x2 G*(v d_s12)   (d_*: see ssim_fwd_kernel)
//
// Mapping: a workgroup of 256 lanes owns a kTH x kTW output tile of one plane (blockIdx.z).  It stages the tile with its
// 5-pixel halo in LDS (zeros outside the image), runs the horizontal pass over the kIH haloed rows into LDS, and the
// vertical pass from LDS with the lane's column in registers: a lane owns kRows consecutive rows of one column, so the
// 11 + kRows - 1 values it loads serve kRows outputs.  Every output is written once by one lane: no atomics, the same
// bits on every run, and the bits of a plane do not depend on the batch around it or on the strides it is read through.
// LDS: the haloed rows have an odd pitch (kIS = 43), the horizontal results a pitch of kTW = 32; in both passes the 32
// lanes of a ds_read_b32 group read 32 consecutive dwords (32 banks), and the two halves of a wave never conflict.
// Inputs are read -- and v_img1 is written -- through element strides (NCHW, or the permute(0, 3, 1, 2) view of
// [B, H, W, C]); S, the three derivative maps and v are contiguous NCHW.
// Roundings per moment: 11 in each of the two fmaf chains, one per pass for the fp32 window constant, one for the
// product under the blur = 25 (edgegaussians_amd/ssim.py, tests/ssim_util.py: K).
#include "common.h"

using namespace eg;

namespace {

constexpr int kTW = 32, kTH = 32;  // output tile (edgegaussians_amd/ssim.py: TILE_W, TILE_H)
constexpr int kR = 5, kTaps = 2 * kR + 1;
constexpr int kIW = kTW + 2 * kR, kIH = kTH + 2 * kR;  // the haloed tile
constexpr int kIS = kIW + 1;                           // its LDS row pitch (odd)
constexpr int kThreads = 256;
constexpr int kRows = kTH / (kThreads / kTW);  // output rows per lane in the vertical pass
static_assert(kTW == 32 && kThreads % kTW == 0 && kTH % (kThreads / kTW) == 0, "lane = (column, group of kRows rows)");
constexpr float kC1 = 0.0001f, kC2 = 0.0009f;  // 0.01^2, 0.03^2

// float32 of exp(-(k - 5)^2 / (2 1.5^2)) / sum, k = 0..10, normalised in float64 (tests/test_ssim_host.py reads this line)
#define EG_SSIM_WINDOW 0.001028380123898387f, 0.0075987582094967365f, 0.036000773310661316f, 0.10936068743467331f, 0.21300554275512695f, 0.26601171493530273f, 0.21300554275512695f, 0.10936068743467331f, 0.036000773310661316f, 0.0075987582094967365f, 0.001028380123898387f

struct Strides {
  int64_t b, c, h, w;
};

// vertical pass of one horizontal-pass image (pitch kTW): the lane's kRows outputs of column tx, rows ty kRows ..
__device__ __forceinline__ void blur_column(const float *__restrict__ img, int tx, int ty, float *out) {
  constexpr float g[kTaps] = {EG_SSIM_WINDOW};
  const float *col = img + ty * kRows * kTW + tx;
  float v[kRows + kTaps - 1];
#pragma unroll
  for (int j = 0; j < kRows + kTaps - 1; ++j) v[j] = col[j * kTW];
#pragma unroll
  for (int i = 0; i < kRows; ++i) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) acc = fmaf(g[k], v[i + k], acc);
    out[i] = acc;
  }
}

__global__ void __launch_bounds__(kThreads)
ssim_fwd_kernel(const float *__restrict__ img1, const float *__restrict__ img2, int C, int H, int W, Strides st1,
                Strides st2, float *__restrict__ S, float *__restrict__ d_m1, float *__restrict__ d_s1,
                float *__restrict__ d_s12) {
  constexpr float g[kTaps] = {EG_SSIM_WINDOW};
  __shared__ float tile[2][kIH * kIS];
  __shared__ float hor[5][kIH * kTW];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const int plane = blockIdx.z, b = plane / C, c = plane - b * C;
  const float *p1 = img1 + b * st1.b + c * st1.c, *p2 = img2 + b * st2.b + c * st2.c;
  for (int idx = tid; idx < kIH * kIW; idx += kThreads) {
    const int r = idx / kIW, q = idx - r * kIW;
    const int y = y0 - kR + r, x = x0 - kR + q;
    float a = 0.f, bb = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      a = p1[y * st1.h + x * st1.w];
      bb = p2[y * st2.h + x * st2.w];
    }
    tile[0][r * kIS + q] = a;
    tile[1][r * kIS + q] = bb;
  }
  __syncthreads();
  for (int idx = tid; idx < kIH * kTW; idx += kThreads) {
    const int r = idx / kTW, q = idx - r * kTW;
    const float *t1 = tile[0] + r * kIS + q, *t2 = tile[1] + r * kIS + q;
    float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const float a = t1[k], bb = t2[k];
      m1 = fmaf(g[k], a, m1);
      m2 = fmaf(g[k], bb, m2);
      e11 = fmaf(g[k], a * a, e11);
      e22 = fmaf(g[k], bb * bb, e22);
      e12 = fmaf(g[k], a * bb, e12);
    }
    hor[0][idx] = m1, hor[1][idx] = m2, hor[2][idx] = e11, hor[3][idx] = e22, hor[4][idx] = e12;
  }
  __syncthreads();
  const int tx = tid % kTW, ty = tid / kTW;
  float mom[5][kRows];
#pragma unroll
  for (int m = 0; m < 5; ++m) blur_column(hor[m], tx, ty, mom[m]);
  const int x = x0 + tx;
  if (x >= W) return;
#pragma unroll
  for (int i = 0; i < kRows; ++i) {
    const int y = y0 + ty * kRows + i;
    if (y >= H) break;
    const float m1 = mom[0][i], m2 = mom[1][i];
    const float s1 = mom[2][i] - m1 * m1, s2 = mom[3][i] - m2 * m2, s12 = mom[4][i] - m1 * m2;
    const float A1 = 2.f * m1 * m2 + kC1, A2 = 2.f * s12 + kC2;
    const float B1 = m1 * m1 + m2 * m2 + kC1, B2 = s1 + s2 + kC2;
    const float r1 = 1.f / B1, r2 = 1.f / B2, r12 = r1 * r2;
    const float val = A1 * A2 * r12;
    const size_t o = ((size_t)plane * H + y) * W + x;
    S[o] = val;
    if (d_m1) {
      const float ds1 = -val * r2;            // -A1 A2 / (B1 B2^2)
      const float ds12 = 2.f * A1 * r12;      // 2 A1 / (B1 B2)
      d_m1[o] = 2.f * m2 * A2 * r12 - 2.f * m1 * val * r1 - 2.f * m1 * ds1 - m2 * ds12;
      d_s1[o] = ds1;
      d_s12[o] = ds12;
    }
  }
}

__global__ void __launch_bounds__(kThreads)
ssim_bwd_kernel(const float *__restrict__ img1, const float *__restrict__ img2, int C, int H, int W, Strides st1,
                Strides st2, const float *__restrict__ v, const float *__restrict__ d_m1,
                const float *__restrict__ d_s1, const float *__restrict__ d_s12, float *__restrict__ v_img1) {
  constexpr float g[kTaps] = {EG_SSIM_WINDOW};
  __shared__ float tile[3][kIH * kIS];
  __shared__ float hor[3][kIH * kTW];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const int plane = blockIdx.z, b = plane / C, c = plane - b * C;
  const size_t base = (size_t)plane * H * W;
  for (int idx = tid; idx < kIH * kIW; idx += kThreads) {
    const int r = idx / kIW, q = idx - r * kIW;
    const int y = y0 - kR + r, x = x0 - kR + q;
    float t0 = 0.f, t1 = 0.f, t2 = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const size_t o = base + (size_t)y * W + x;
      const float vv = v[o];
      t0 = vv * d_m1[o], t1 = vv * d_s1[o], t2 = vv * d_s12[o];
    }
    tile[0][r * kIS + q] = t0, tile[1][r * kIS + q] = t1, tile[2][r * kIS + q] = t2;
  }
  __syncthreads();
  for (int idx = tid; idx < kIH * kTW; idx += kThreads) {
    const int r = idx / kTW, q = idx - r * kTW;
    const int o = r * kIS + q;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      a0 = fmaf(g[k], tile[0][o + k], a0);
      a1 = fmaf(g[k], tile[1][o + k], a1);
      a2 = fmaf(g[k], tile[2][o + k], a2);
    }
    hor[0][idx] = a0, hor[1][idx] = a1, hor[2][idx] = a2;
  }
  __syncthreads();
  const int tx = tid % kTW, ty = tid / kTW;
  float blur[3][kRows];
#pragma unroll
  for (int m = 0; m < 3; ++m) blur_column(hor[m], tx, ty, blur[m]);
  const int x = x0 + tx;
  if (x >= W) return;
  const float *p1 = img1 + b * st1.b + c * st1.c, *p2 = img2 + b * st2.b + c * st2.c;
  float *po = v_img1 + b * st1.b + c * st1.c;
#pragma unroll
  for (int i = 0; i < kRows; ++i) {
    const int y = y0 + ty * kRows + i;
    if (y >= H) break;
    const int64_t o1 = y * st1.h + x * st1.w;
    const float a = p1[o1], bb = p2[y * st2.h + x * st2.w];
    po[o1] = blur[0][i] + 2.f * a * blur[1][i] + bb * blur[2][i];
  }
}

// ---- the photometric loss (1 - lambda) mean|x1 - x2| + lambda (1 - mean S) as a scalar (edgegaussians_amd/losses.py):
// with a mean the cotangent of S is one number, so neither S nor a cotangent map is ever written.  The forward is
// ssim_fwd_kernel's tile walk; instead of storing S a workgroup adds its pixels' S (the lane's kRows values in row
// order, the wave's DPP tree, the waves in order) and the |x1 - x2| of its own kTH x kTW tile, which it holds in LDS
// (the lane's four pixels tid, tid + kThreads, .. in order, then the same tree), into its two words of a slab;
// photometric_finalize_kernel (one wave) adds the slab in index order (slab_sum_f).  `crop` = kR states padding="valid":
// only the pixels crop <= y < H - crop, crop <= x < W - crop count in the sum of S, and the derivative maps are zero
// outside them.  Longest addition chain of one S: (kRows - 1) + 6 + 3 + (ceil(G / 64) - 1) + 6, of one |x1 - x2|:
// (kTH kTW / kThreads - 1) + the same (tests/losses_util.py).
constexpr int kFinLanes = 64;
static_assert(kFinLanes == kWave, "slab_sum_f is one wave");

__global__ void __launch_bounds__(kThreads)
photometric_fwd_kernel(const float *__restrict__ img1, const float *__restrict__ img2, int C, int H, int W, Strides st1,
                       Strides st2, int crop, float *__restrict__ d_m1, float *__restrict__ d_s1,
                       float *__restrict__ d_s12, float *__restrict__ slab) {
  constexpr float g[kTaps] = {EG_SSIM_WINDOW};
  __shared__ float tile[2][kIH * kIS];
  __shared__ float hor[5][kIH * kTW];
  __shared__ float wave_s[kThreads / kWave], wave_l[kThreads / kWave];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const int plane = blockIdx.z, b = plane / C, c = plane - b * C;
  const float *p1 = img1 + b * st1.b + c * st1.c, *p2 = img2 + b * st2.b + c * st2.c;
  for (int idx = tid; idx < kIH * kIW; idx += kThreads) {
    const int r = idx / kIW, q = idx - r * kIW;
    const int y = y0 - kR + r, x = x0 - kR + q;
    float a = 0.f, bb = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      a = p1[y * st1.h + x * st1.w];
      bb = p2[y * st2.h + x * st2.w];
    }
    tile[0][r * kIS + q] = a;
    tile[1][r * kIS + q] = bb;
  }
  __syncthreads();
  float l1 = 0.f;  // (pixels outside the image are staged as zeros: a term of 0)
  for (int idx = tid; idx < kTH * kTW; idx += kThreads) {
    const int o = (idx / kTW + kR) * kIS + idx % kTW + kR;
    l1 += fabsf(tile[0][o] - tile[1][o]);
  }
  for (int idx = tid; idx < kIH * kTW; idx += kThreads) {
    const int r = idx / kTW, q = idx - r * kTW;
    const float *t1 = tile[0] + r * kIS + q, *t2 = tile[1] + r * kIS + q;
    float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const float a = t1[k], bb = t2[k];
      m1 = fmaf(g[k], a, m1);
      m2 = fmaf(g[k], bb, m2);
      e11 = fmaf(g[k], a * a, e11);
      e22 = fmaf(g[k], bb * bb, e22);
      e12 = fmaf(g[k], a * bb, e12);
    }
    hor[0][idx] = m1, hor[1][idx] = m2, hor[2][idx] = e11, hor[3][idx] = e22, hor[4][idx] = e12;
  }
  __syncthreads();
  const int tx = tid % kTW, ty = tid / kTW;
  float mom[5][kRows];
#pragma unroll
  for (int m = 0; m < 5; ++m) blur_column(hor[m], tx, ty, mom[m]);
  const int x = x0 + tx;
  float ssum = 0.f;
#pragma unroll
  for (int i = 0; i < kRows; ++i) {
    const int y = y0 + ty * kRows + i;
    const float m1 = mom[0][i], m2 = mom[1][i];
    const float s1 = mom[2][i] - m1 * m1, s2 = mom[3][i] - m2 * m2, s12 = mom[4][i] - m1 * m2;
    const float A1 = 2.f * m1 * m2 + kC1, A2 = 2.f * s12 + kC2;
    const float B1 = m1 * m1 + m2 * m2 + kC1, B2 = s1 + s2 + kC2;
    const float r1 = 1.f / B1, r2 = 1.f / B2, r12 = r1 * r2;
    const float val = A1 * A2 * r12;
    const bool counted = x >= crop && x < W - crop && y >= crop && y < H - crop;
    ssum += counted ? val : 0.f;
    if (d_m1 && x < W && y < H) {
      const float ds1 = -val * r2;            // -A1 A2 / (B1 B2^2)
      const float ds12 = 2.f * A1 * r12;      // 2 A1 / (B1 B2)
      const size_t o = ((size_t)plane * H + y) * W + x;
      d_m1[o] = counted ? 2.f * m2 * A2 * r12 - 2.f * m1 * val * r1 - 2.f * m1 * ds1 - m2 * ds12 : 0.f;
      d_s1[o] = counted ? ds1 : 0.f;
      d_s12[o] = counted ? ds12 : 0.f;
    }
  }
  const float ssum_wg = block_sum_f<kThreads>(ssum, wave_s), l1_wg = block_sum_f<kThreads>(l1, wave_l);
  if (tid == 0) {
    const size_t wg = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    slab[2 * wg] = ssum_wg, slab[2 * wg + 1] = l1_wg;
  }
}

// out[0] = (1 - lambda) out[1] + lambda (1 - out[2]), out[1] = mean |x1 - x2|, out[2] = mean S
__global__ void __launch_bounds__(kFinLanes)
photometric_finalize_kernel(const float *__restrict__ slab, int G, float lambda, float n, float n_s,
                            float *__restrict__ out) {
  const float ssum = slab_sum_f(slab, G, 2), l1 = slab_sum_f(slab + 1, G, 2);
  if (threadIdx.x == kFinLanes - 1) {
    const float l1_mean = l1 / n, s_mean = ssum / n_s;
    out[0] = (1.f - lambda) * l1_mean + lambda * (1.f - s_mean), out[1] = l1_mean, out[2] = s_mean;
  }
}

// v_x1 = (1 - lambda) (v / n) sign(x1 - x2) - lambda (v / n_s) (G*d_m1 + 2 x1 G*d_s1 + x2 G*d_s12): ssim_bwd_kernel's
// tile walk on the derivative maps themselves; v is one number on the device
__global__ void __launch_bounds__(kThreads)
photometric_bwd_kernel(const float *__restrict__ img1, const float *__restrict__ img2, int C, int H, int W, Strides st1,
                       Strides st2, float lambda, float n, float n_s, const float *__restrict__ v,
                       const float *__restrict__ d_m1, const float *__restrict__ d_s1, const float *__restrict__ d_s12,
                       float *__restrict__ v_img1) {
  constexpr float g[kTaps] = {EG_SSIM_WINDOW};
  __shared__ float tile[3][kIH * kIS];
  __shared__ float hor[3][kIH * kTW];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const int plane = blockIdx.z, b = plane / C, c = plane - b * C;
  const size_t base = (size_t)plane * H * W;
  for (int idx = tid; idx < kIH * kIW; idx += kThreads) {
    const int r = idx / kIW, q = idx - r * kIW;
    const int y = y0 - kR + r, x = x0 - kR + q;
    float t0 = 0.f, t1 = 0.f, t2 = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const size_t o = base + (size_t)y * W + x;
      t0 = d_m1[o], t1 = d_s1[o], t2 = d_s12[o];
    }
    tile[0][r * kIS + q] = t0, tile[1][r * kIS + q] = t1, tile[2][r * kIS + q] = t2;
  }
  __syncthreads();
  for (int idx = tid; idx < kIH * kTW; idx += kThreads) {
    const int r = idx / kTW, q = idx - r * kTW;
    const int o = r * kIS + q;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      a0 = fmaf(g[k], tile[0][o + k], a0);
      a1 = fmaf(g[k], tile[1][o + k], a1);
      a2 = fmaf(g[k], tile[2][o + k], a2);
    }
    hor[0][idx] = a0, hor[1][idx] = a1, hor[2][idx] = a2;
  }
  __syncthreads();
  const int tx = tid % kTW, ty = tid / kTW;
  float blur[3][kRows];
#pragma unroll
  for (int m = 0; m < 3; ++m) blur_column(hor[m], tx, ty, blur[m]);
  const int x = x0 + tx;
  if (x >= W) return;
  const float *p1 = img1 + b * st1.b + c * st1.c, *p2 = img2 + b * st2.b + c * st2.c;
  float *po = v_img1 + b * st1.b + c * st1.c;
  const float vv = v[0];
  const float k_l1 = (1.f - lambda) * (vv / n), k_s = lambda * (vv / n_s);  // (lambda = 0: v / n, the pointwise L1's scale)
#pragma unroll
  for (int i = 0; i < kRows; ++i) {
    const int y = y0 + ty * kRows + i;
    if (y >= H) break;
    const int64_t o1 = y * st1.h + x * st1.w;
    const float a = p1[o1], bb = p2[y * st2.h + x * st2.w];
    const float d = a - bb, sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : d);
    po[o1] = k_l1 * sgn - k_s * (blur[0][i] + 2.f * a * blur[1][i] + bb * blur[2][i]);
  }
}

// the checks both entries share
#define EG_SSIM_CHECK()                                                                                         \
  do {                                                                                                          \
    EG_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1, "bad sizes (B, C, H, W >= 1)");                            \
    EG_REQUIRE((int64_t)B * C <= 65535, "B * C must fit the grid (<= 65535 planes)");                           \
    EG_REQUIRE(cdiv(H, kTH) <= 65535 && W <= (1 << 24), "H, W must fit the grid (H <= 65535 * 32, W <= 2^24)"); \
    EG_REQUIRE(img1 && img2, "null img1 / img2");                                                               \
    EG_REQUIRE(strides1 && strides2, "null strides1 / strides2");                                               \
    for (int i = 0; i < 4; ++i) EG_REQUIRE(strides1[i] >= 0 && strides2[i] >= 0, "negative stride");            \
  } while (0)

}  // namespace

extern "C" int eg_ssim_fwd(const float *img1, const float *img2, int32_t B, int32_t C, int32_t H, int32_t W,
                           const int64_t *strides1, const int64_t *strides2, float *S, float *d_m1, float *d_s1,
                           float *d_s12, eg_stream_t stream) {
  EG_SSIM_CHECK();
  EG_REQUIRE(S, "null S");
  EG_REQUIRE((d_m1 && d_s1 && d_s12) || (!d_m1 && !d_s1 && !d_s12), "d_m1, d_s1, d_s12: all three or none");
  const Strides st1 = {strides1[0], strides1[1], strides1[2], strides1[3]};
  const Strides st2 = {strides2[0], strides2[1], strides2[2], strides2[3]};
  const dim3 grid(cdiv(W, kTW), cdiv(H, kTH), B * C);
  ssim_fwd_kernel<<<grid, kThreads, 0, as_stream(stream)>>>(img1, img2, C, H, W, st1, st2, S, d_m1, d_s1, d_s12);
  return check_launch("ssim_fwd");
}

extern "C" int eg_ssim_bwd(const float *img1, const float *img2, int32_t B, int32_t C, int32_t H, int32_t W,
                           const int64_t *strides1, const int64_t *strides2, const float *v, const float *d_m1,
                           const float *d_s1, const float *d_s12, float *v_img1, eg_stream_t stream) {
  EG_SSIM_CHECK();
  EG_REQUIRE(v && d_m1 && d_s1 && d_s12, "null v / d_m1 / d_s1 / d_s12");
  EG_REQUIRE(v_img1, "null v_img1");
  const Strides st1 = {strides1[0], strides1[1], strides1[2], strides1[3]};
  const Strides st2 = {strides2[0], strides2[1], strides2[2], strides2[3]};
  const dim3 grid(cdiv(W, kTW), cdiv(H, kTH), B * C);
  ssim_bwd_kernel<<<grid, kThreads, 0, as_stream(stream)>>>(img1, img2, C, H, W, st1, st2, v, d_m1, d_s1, d_s12, v_img1);
  return check_launch("ssim_bwd");
}

// number of map elements the mean of S runs over: all of them, or the crop by kR on every side
static int64_t map_elements(int64_t planes, int H, int W, int crop) { return planes * (H - 2 * crop) * (W - 2 * crop); }

extern "C" int eg_photometric_fwd(const float *img1, const float *img2, int32_t B, int32_t C, int32_t H, int32_t W,
                                  const int64_t *strides1, const int64_t *strides2, int32_t valid, float lambda,
                                  float *d_m1, float *d_s1, float *d_s12, float *slab, int64_t slab_len, float *out,
                                  eg_stream_t stream) {
  EG_SSIM_CHECK();
  EG_REQUIRE(!valid || (H >= kTaps && W >= kTaps), "valid needs H, W >= 11");
  EG_REQUIRE((d_m1 && d_s1 && d_s12) || (!d_m1 && !d_s1 && !d_s12), "d_m1, d_s1, d_s12: all three or none");
  const dim3 grid(cdiv(W, kTW), cdiv(H, kTH), B * C);
  const int64_t G = (int64_t)grid.x * grid.y * grid.z;
  EG_REQUIRE(G <= INT32_MAX, "too many workgroups for the slab (< 2^31)");
  EG_REQUIRE(slab && out, "null slab / out");
  EG_REQUIRE(slab_len >= 2 * G, "slab too small (two floats per 32 x 32 tile of every plane)");
  const Strides st1 = {strides1[0], strides1[1], strides1[2], strides1[3]};
  const Strides st2 = {strides2[0], strides2[1], strides2[2], strides2[3]};
  const int crop = valid ? kR : 0;
  const int64_t planes = (int64_t)B * C;
  photometric_fwd_kernel<<<grid, kThreads, 0, as_stream(stream)>>>(img1, img2, C, H, W, st1, st2, crop, d_m1, d_s1,
                                                                   d_s12, slab);
  photometric_finalize_kernel<<<1, kFinLanes, 0, as_stream(stream)>>>(
      slab, (int)G, lambda, (float)(planes * H * W), (float)map_elements(planes, H, W, crop), out);
  return check_launch("photometric_fwd");
}

extern "C" int eg_photometric_bwd(const float *img1, const float *img2, int32_t B, int32_t C, int32_t H, int32_t W,
                                  const int64_t *strides1, const int64_t *strides2, int32_t valid, float lambda,
                                  const float *v, const float *d_m1, const float *d_s1, const float *d_s12,
                                  float *v_img1, eg_stream_t stream) {
  EG_SSIM_CHECK();
  EG_REQUIRE(!valid || (H >= kTaps && W >= kTaps), "valid needs H, W >= 11");
  EG_REQUIRE(v && d_m1 && d_s1 && d_s12, "null v / d_m1 / d_s1 / d_s12");
  EG_REQUIRE(v_img1, "null v_img1");
  const Strides st1 = {strides1[0], strides1[1], strides1[2], strides1[3]};
  const Strides st2 = {strides2[0], strides2[1], strides2[2], strides2[3]};
  const dim3 grid(cdiv(W, kTW), cdiv(H, kTH), B * C);
  const int64_t planes = (int64_t)B * C;
  photometric_bwd_kernel<<<grid, kThreads, 0, as_stream(stream)>>>(
      img1, img2, C, H, W, st1, st2, lambda, (float)(planes * H * W), (float)map_elements(planes, H, W, valid ? kR : 0), v,
      d_m1, d_s1, d_s12, v_img1);
  return check_launch("photometric_bwd");
}
