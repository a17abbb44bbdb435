// Compositing of colours of any channel count (rasterization(colors=[..., D]) with D other than 1 or 3): the classic
// one-workgroup-per-tile walk of composite.hip for chunks of up to 32 channels.
//
// A call composites ONE chunk of `n_real` channels that lives inside full-width tensors: colors / v_colors /
// backgrounds are addressed with the row stride `cs`, render / v_render with the row stride `ps`, so the caller passes
// pointers to the chunk's first channel and never copies.  The kernels are instantiated for CH = 2, 4, 8, 16, 32; a
// narrower chunk runs in the next width up, its padding channels staged as exact zeros and never loaded from or
// written to global memory (n_real guards every load, store and atomic).
//
// Forward: the per-pixel walk of composite_fwd_kernel with the same source expressions for sigma, the threshold skip,
// alpha, the 1/255 cut and the transmittance stop, so alphas and last_ids do not depend on the width or on how a call
// is cut into chunks.  The colour rows of a 256-Gaussian batch are staged through LDS by the whole workgroup, one
// 16-byte unit per lane (consecutive lanes fetch consecutive units of a row: coalesced loads, conflict-free
// ds_write_b128); the walk reads them back as broadcast ds_read_b128.
//
// Backward: the walk of composite_bwd_colors_kernel.  Its reduction -- one six-step butterfly per partial, then lane 0
// issuing every atomic -- costs 6 (8 + CH + 1) cross-lane operations and 8 + CH + 1 serial atomics per (wave,
// Gaussian).  Here the CH colour partials and the 8 splat-side partials are reduced by a HALVING EXCHANGE
// (lane_transpose_sum, wide_dev.h): in a step over lane bit b a lane keeps one half of its values, hands the other half to
// lane ^ (1 << b) and adds what it receives, so n values cost n/2 + n/4 + ... + 1 = n - 1 exchanges and finish with
// component k in lane k.  Lanes 0 .. CH-1 then hold the colour sums, lanes 32 .. 39 the splat-side sums and lane 63
// the depth sum, and ONE atomic instruction adds them all: consecutive lanes to consecutive addresses.  Measured
// against the plain scheme instantiated at the same widths (profiles/channels_bwd_reduction_ab.jsonl).
#include "common.h"
#include "wide_dev.h"

namespace eg {

template <int CH, bool DEPTH, bool BG>
__global__ void __launch_bounds__(256)
composite_fwd_wide_kernel(const float4 *__restrict__ splat, const float *__restrict__ colors,
                          const int *__restrict__ offsets, const int *__restrict__ flat, int width, int height, int tw,
                          int th, float *__restrict__ render, float *__restrict__ alphas, int *__restrict__ last_ids,
                          const WideArgs wa) {
  __shared__ float4 sA[kTilePix];  // x, y, a, b
  __shared__ float4 sB[kTilePix];  // c, o, sigma threshold, depth (DEPTH)
  __shared__ __attribute__((aligned(16))) float sC[kTilePix * CH];

  {
    const int c = blockIdx.y, T = tw * th;
    const size_t hw = (size_t)width * height;
    flat += wide_list_base(offsets, T, c);
    offsets += (size_t)c * (T + 1);
    splat += 2 * (size_t)wa.N * c;
    if (wa.colors_per_camera) colors += (size_t)wa.N * wa.cs * c;
    render += hw * wa.ps * c;
    if (alphas) alphas += hw * c;
    if (last_ids) last_ids += hw * c;
  }
  const int tile = xcd_tile(blockIdx.x, tw * th);
  const int tid = threadIdx.x;
  const int ty = tile / tw, tx = tile - ty * tw;
  const int i = ty * kTile + (tid >> 4), j = tx * kTile + (tid & 15);
  const bool inside = (i < height) && (j < width);
  const float px = (float)j + 0.5f, py = (float)i + 0.5f;
  const int start = offsets[tile], end = offsets[tile + 1];

  float T = 1.f;
  float pix[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) pix[k] = 0.f;
  float pix_d = 0.f;
  int last = 0;
  bool done = !inside;

  for (int base = start; base < end; base += kTilePix) {
    if (__syncthreads_and(done)) break;
    const int idx = base + tid;
    const int n = min(kTilePix, end - base);
    if (idx < end) {
      const int g = flat[idx];
      const float4 s0 = splat[2 * g], s1 = splat[2 * g + 1];
      sA[tid] = s0;
      sB[tid] = make_float4(s1.x, s1.y, __logf(255.f * s1.y) + kThrMargin, DEPTH ? s1.z : 0.f);
    }
    stage_colors<CH>(sC, colors, flat, base, 1, n, wa);
    __syncthreads();
    for (int t = 0; t < n && !done; ++t) {
      const float4 A = sA[t], B = sB[t];
      const float dx = A.x - px, dy = A.y - py;
      const float sigma = 0.5f * (A.z * dx * dx + B.x * dy * dy) + A.w * dx * dy;
      if (sigma < 0.f || sigma > B.z) continue;
      const float alpha = fminf(kAlphaMax, B.y * __expf(-sigma));
      if (alpha < kAlphaMin) continue;
      const float next_T = T * (1.f - alpha);
      if (next_T <= kTStop) { done = true; break; }
      const float w = alpha * T;
#pragma unroll
      for (int k = 0; k < CH; ++k) pix[k] += sC[t * CH + k] * w;
      if constexpr (DEPTH) pix_d += B.w * w;
      last = base + t;
      T = next_T;
    }
  }

  if (inside) {
    const int p = i * width + j;
    if (alphas) alphas[p] = 1.f - T;
    if (last_ids) last_ids[p] = last;
    float *out = render + (size_t)p * wa.ps;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      if (k < wa.n_real) {
        float v = pix[k];
        if constexpr (BG) v += T * wa.bg[(size_t)blockIdx.y * wa.cs + k];
        out[k] = v;
      }
    }
    if constexpr (DEPTH) out[wa.n_real] = pix_d;  // (the depth channel's background is 0)
  }
}

template <int CH, bool DEPTH, bool BG>
__global__ void __launch_bounds__(256)
composite_bwd_wide_kernel(const float4 *__restrict__ splat, const float *__restrict__ colors,
                          const int *__restrict__ offsets, const int *__restrict__ flat, int width, int height, int tw,
                          int th, const float *__restrict__ alphas, const int *__restrict__ last_ids,
                          const float *__restrict__ v_render, const float *__restrict__ v_alphas,
                          float *__restrict__ g2d, float *__restrict__ v_colors, const WideArgs wa) {
  __shared__ float4 sA[kTilePix];
  __shared__ float4 sB[kTilePix];  // c, o, depth (DEPTH), Gaussian id (int bits)
  __shared__ __attribute__((aligned(16))) float sC[kTilePix * CH];

  {
    const int c = blockIdx.y, T = tw * th;
    const size_t hw = (size_t)width * height, n = (size_t)wa.N;
    flat += wide_list_base(offsets, T, c);
    offsets += (size_t)c * (T + 1);
    splat += 2 * n * c;
    if (wa.colors_per_camera) colors += n * wa.cs * c;
    alphas += hw * c;
    last_ids += hw * c;
    v_render += hw * wa.ps * c;
    if (v_alphas) v_alphas += hw * c;
    g2d += 8 * n * c;
    if (v_colors) v_colors += n * wa.cs * c;
  }
  const int tile = xcd_tile(blockIdx.x, tw * th);
  const int start = offsets[tile], end = offsets[tile + 1];
  if (end <= start) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int ty = tile / tw, tx = tile - ty * tw;
  const int i = ty * kTile + (tid >> 4), j = tx * kTile + (tid & 15);
  const bool inside = (i < height) && (j < width);
  const float px = (float)j + 0.5f, py = (float)i + 0.5f;
  const int p = inside ? i * width + j : 0;

  const float T_final = inside ? 1.f - alphas[p] : 1.f;
  float T = T_final;
  float buffer[CH], vr[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    buffer[k] = 0.f;
    vr[k] = (inside && k < wa.n_real) ? v_render[(size_t)p * wa.ps + k] : 0.f;
  }
  float buffer_d = 0.f, vr_d = 0.f;  // the depth channel (DEPTH)
  if constexpr (DEPTH) vr_d = inside ? v_render[(size_t)p * wa.ps + wa.n_real] : 0.f;
  float bg_vr = 0.f;  // sum_k bg[k] v_render[k] (BG)
  if constexpr (BG) {
#pragma unroll
    for (int k = 0; k < CH; ++k)
      if (k < wa.n_real) bg_vr += wa.bg[(size_t)blockIdx.y * wa.cs + k] * vr[k];
  }
  const float va_pix = (inside && v_alphas) ? v_alphas[p] : 0.f;
  // a pixel nothing contributed to has alpha == 0 exactly; mark it with last = -1
  const int bin_final = (inside && alphas[p] > 0.f) ? last_ids[p] : -1;
  int wave_last = bin_final;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) wave_last = max(wave_last, __shfl_xor(wave_last, d, 64));

  const int n_batches = (end - start + kTilePix - 1) / kTilePix;
  for (int b = 0; b < n_batches; ++b) {
    __syncthreads();
    const int batch_end = end - 1 - kTilePix * b;
    const int size = min(kTilePix, batch_end + 1 - start);
    const int idx = batch_end - tid;
    if (idx >= start) {
      const int g = flat[idx];
      const float4 s0 = splat[2 * g], s1 = splat[2 * g + 1];
      sA[tid] = s0;
      sB[tid] = make_float4(s1.x, s1.y, DEPTH ? s1.z : 0.f, __int_as_float(g));
    }
    stage_colors<CH>(sC, colors, flat, batch_end, -1, size, wa);
    __syncthreads();
    for (int t = max(0, batch_end - wave_last); t < size; ++t) {
      bool valid = inside && (batch_end - t <= bin_final);
      const float4 A = sA[t], B = sB[t];
      const float dx = A.x - px, dy = A.y - py;
      float vis = 0.f, alpha = 0.f;
      if (valid) {
        const float sigma = 0.5f * (A.z * dx * dx + B.x * dy * dy) + A.w * dx * dy;
        vis = __expf(-sigma);
        alpha = fminf(kAlphaMax, B.y * vis);
        if (sigma < 0.f || alpha < kAlphaMin) valid = false;
      }
      if (!__any(valid)) continue;
      float r_rgb[CH];
#pragma unroll
      for (int k = 0; k < CH; ++k) r_rgb[k] = 0.f;
      float r_d = 0.f;
      float gv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // g2d record: gx gy |gx| |gy| ga gb gc go
      if (valid) {
        const float ra = 1.f / (1.f - alpha);
        T *= ra;
        const float fac = alpha * T;
        float v_alpha = 0.f;
#pragma unroll
        for (int k = 0; k < CH; ++k) {
          r_rgb[k] = fac * vr[k];
          v_alpha += (sC[t * CH + k] * T - buffer[k] * ra) * vr[k];
        }
        if constexpr (DEPTH) {
          r_d = fac * vr_d;
          v_alpha += (B.z * T - buffer_d * ra) * vr_d;
        }
        v_alpha += T_final * ra * va_pix;
        if constexpr (BG) v_alpha += -T_final * ra * bg_vr;
        if (B.y * vis <= kAlphaMax) {
          const float v_sigma = -B.y * vis * v_alpha;
          gv[0] = v_sigma * (A.z * dx + A.w * dy);
          gv[1] = v_sigma * (A.w * dx + B.x * dy);
          gv[2] = fabsf(gv[0]);
          gv[3] = fabsf(gv[1]);
          gv[4] = 0.5f * v_sigma * dx * dx;
          gv[5] = v_sigma * dx * dy;
          gv[6] = 0.5f * v_sigma * dy * dy;
          gv[7] = vis * v_alpha;
        }
#pragma unroll
        for (int k = 0; k < CH; ++k) buffer[k] += sC[t * CH + k] * fac;
        if constexpr (DEPTH) buffer_d += B.z * fac;
      }
      const int g = __float_as_int(B.w);
      // component k of the colour sums in lane k (k < CH), of the splat-side sums in lane 32 + k
      const float c_sum = lane_transpose_sum<CH>(r_rgb, lane);
      const float g_sum = lane_transpose_sum<8>(gv, lane);
      float *dst = nullptr;
      float val = 0.f;
      if (lane < 32) {
        if (v_colors && lane < wa.n_real) { dst = v_colors + (size_t)g * wa.cs + lane; val = c_sum; }
      } else if (lane < 40) {
        dst = g2d + (size_t)g * 8 + (lane - 32);
        val = g_sum;
      }
      if constexpr (DEPTH) {
        r_d = wave_sum_dpp_f(r_d);  // (the sum lands in lane 63)
        if (lane == 63) { dst = wa.v_depths + (size_t)blockIdx.y * wa.N + g; val = r_d; }
      }
      if (dst) unsafeAtomicAdd(dst, val);
    }
  }
}

}  // namespace eg

using namespace eg;

// ---------------------------------------------------------------------------------------------
// (macros, not functions: the error message names the entry point)
#define EG_WIDE_CHECK(C, N, channels, n_real, depth, width, height, cs, ps)                                  \
  EG_REQUIRE(C >= 1 && C <= 65535 && N >= 0 && width > 0 && height > 0, "bad sizes");                         \
  EG_REQUIRE(channels >= 1 && channels <= 32, "channels (the chunk width) must be 1 .. 32");                  \
  EG_REQUIRE(n_real >= 1 && n_real <= channels, "n_real must be 1 .. channels");                              \
  EG_REQUIRE(cs >= n_real, "color_stride is smaller than the channel count");                                 \
  EG_REQUIRE(ps >= n_real + (depth ? 1 : 0), "pixel_stride is smaller than the channel count")

#define EG_WIDE_DB(LAUNCH, CH)                                                  \
  do {                                                                          \
    if (depth) { if (bg) LAUNCH(CH, true, true); else LAUNCH(CH, true, false); } \
    else { if (bg) LAUNCH(CH, false, true); else LAUNCH(CH, false, false); }     \
  } while (0)

#define EG_WIDE_DISPATCH(LAUNCH)                   \
  do {                                             \
    if (channels <= 2) EG_WIDE_DB(LAUNCH, 2);      \
    else if (channels <= 4) EG_WIDE_DB(LAUNCH, 4); \
    else if (channels <= 8) EG_WIDE_DB(LAUNCH, 8); \
    else if (channels <= 16) EG_WIDE_DB(LAUNCH, 16); \
    else EG_WIDE_DB(LAUNCH, 32);                   \
  } while (0)

// the colour rows can be fetched in 16-byte (CH = 2: 8-byte) units
static int wide_rows_aligned(const float *colors, int channels, int cs) {
  const int vw = channels <= 2 ? 2 : 4;
  return ((uintptr_t)colors % (vw * sizeof(float)) == 0) && (cs % vw == 0);
}

extern "C" int eg_composite_fwd_wide_cams(int32_t C, const float *splat, int32_t N, const float *colors,
                                          int32_t colors_per_camera, int32_t channels, int32_t depth,
                                          const float *backgrounds, const int32_t *offsets,
                                          const int32_t *flatten_ids, int32_t width, int32_t height, float *render,
                                          float *alphas, int32_t *last_ids, int32_t n_real, int32_t color_stride,
                                          int32_t pixel_stride, eg_stream_t stream) {
  EG_WIDE_CHECK(C, N, channels, n_real, depth, width, height, color_stride, pixel_stride);
  EG_REQUIRE(colors, "null colors (channels > 0)");
  EG_REQUIRE(splat && offsets && flatten_ids && render, "null pointer");
  const int tw = cdiv(width, kTile), th = cdiv(height, kTile);
  const float *bg = backgrounds;
  const WideArgs wa = {bg, nullptr, N, colors_per_camera != 0, n_real, color_stride, pixel_stride,
                       wide_rows_aligned(colors, channels, color_stride)};
  hipStream_t s = as_stream(stream);
#define EG_LAUNCH_FWD_WIDE(CH, DEPTH, BG)                                                                       \
  composite_fwd_wide_kernel<CH, DEPTH, BG><<<dim3(tw * th, C), 256, 0, s>>>(                                    \
      (const float4 *)splat, colors, offsets, flatten_ids, width, height, tw, th, render, alphas, last_ids, wa)
  EG_WIDE_DISPATCH(EG_LAUNCH_FWD_WIDE);
#undef EG_LAUNCH_FWD_WIDE
  return check_launch("composite_fwd_wide_cams");
}

extern "C" int eg_composite_bwd_wide_cams(int32_t C, const float *splat, int32_t N, const float *colors,
                                          int32_t colors_per_camera, int32_t channels, int32_t depth,
                                          const float *backgrounds, const int32_t *offsets,
                                          const int32_t *flatten_ids, int32_t width, int32_t height,
                                          const float *alphas, const int32_t *last_ids, const float *v_render,
                                          const float *v_alphas, float *g2d, float *v_colors, float *v_depths,
                                          int32_t n_real, int32_t color_stride, int32_t pixel_stride,
                                          eg_stream_t stream) {
  EG_WIDE_CHECK(C, N, channels, n_real, depth, width, height, color_stride, pixel_stride);
  EG_REQUIRE(colors, "null colors (channels > 0)");
  EG_REQUIRE(splat && offsets && flatten_ids && alphas && last_ids && v_render && g2d, "null pointer");
  EG_REQUIRE(!depth || v_depths, "null v_depths (depth channel)");
  const int tw = cdiv(width, kTile), th = cdiv(height, kTile);
  const float *bg = backgrounds;
  const WideArgs wa = {bg, v_depths, N, colors_per_camera != 0, n_real, color_stride, pixel_stride,
                       wide_rows_aligned(colors, channels, color_stride)};
  hipStream_t s = as_stream(stream);
#define EG_LAUNCH_BWD_WIDE(CH, DEPTH, BG)                                                                       \
  composite_bwd_wide_kernel<CH, DEPTH, BG><<<dim3(tw * th, C), 256, 0, s>>>(                                    \
      (const float4 *)splat, colors, offsets, flatten_ids, width, height, tw, th, alphas, last_ids, v_render,      \
      v_alphas, g2d, v_colors, wa)
  EG_WIDE_DISPATCH(EG_LAUNCH_BWD_WIDE);
#undef EG_LAUNCH_BWD_WIDE
  return check_launch("composite_bwd_wide_cams");
}
#undef EG_WIDE_DISPATCH
#undef EG_WIDE_DB
#undef EG_WIDE_CHECK
