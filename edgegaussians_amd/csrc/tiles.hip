// The entries of rasterization(tile_size=8 | 32) and the chunked compositing kernels, templated on the tile size, for
// tiles of 8, 16 and 32 pixels.  At tile_size = 16 D = 1, 3 and the depth-only modes are composited by composite.hip;
// colours of any other channel count come here (eg_composite_{fwd,bwd}_wide_cams).
//
// Binning.  eg_tile_count_ts / eg_tile_emit_sort_ts run the general path's one counting kernel, one emission kernel and
// one per-camera step (binning.hip: launch_tile_count, bin_camera) with the tile size as an argument; the scan
// (eg_tile_offsets_cams) and the per-tile sort know the tile size only through T.  The cameras' Gaussians are addressed
// through a host array of C + 1 range bounds, which serves both layouts of the projection: [c N, (c + 1) N) for the
// dense [C, N, ...] arrays, indptr for the packed lists.  The entries here refuse 16: that size has eg_tile_count,
// eg_tile_emit_sort_cams and eg_packed_bin.
//
// Compositing: one kernel family <TS, CH, DEPTH, BG>.  A call composites ONE chunk of `n_real` channels that lives
// inside full-width tensors: colors / v_colors / backgrounds are addressed with the row stride `cs`, render / v_render
// with the row stride `ps`, so the caller passes pointers to the chunk's first channel and never copies.  CH = 2, 4, 8,
// 16, 32; a narrower chunk runs in the next width up, its padding channels staged as exact zeros and never loaded from
// or written to global memory (n_real guards every load, store and atomic).  CH = 0 (tiles of 8 and 32 only) is the
// depth-only form, which stages no colours.
//
// Forward: the per-pixel walk of composite_fwd_kernel (composite.hip) with the same source expressions for sigma, the
// threshold skip, alpha, the 1/255 cut and the transmittance stop, so alphas and last_ids do not depend on the width or
// on how a call is cut into chunks.  The colour rows of a batch are staged through LDS by the whole workgroup, one
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
//
//   ts = 16  ONE 256-THREAD WORKGROUP PER TILE, one pixel per thread, kStage32 = 256 Gaussians per batch: the shape of
//            the classic kernels of composite.hip.
//   ts = 8   a tile is 64 pixels = one wave: ONE 64-LANE WORKGROUP PER TILE.  The wave stages kStage8 = 128 Gaussians per
//            batch (two per lane) and walks them; a barrier of a one-wave workgroup costs nothing, and no wave ever waits
//            for the list of another tile (four tiles per 256-thread workgroup would hold the three short lists' waves --
//            and their LDS -- until the longest is done, or need wave-private staging without workgroup barriers).
//   ts = 32  a tile is 1024 pixels: ONE 256-THREAD WORKGROUP PER 16 x 16 QUADRANT, four workgroups walking the parent
//            tile's list (kStage32 = 256 per batch).  A 1024-thread workgroup would run 4 waves per SIMD and cap the
//            kernel at 128 VGPRs, below what the backward needs at CH = 32 (three 32-float arrays per lane); the
//            quadrant form keeps the register budget and the code shape of the 16-pixel kernels, its quadrants leave
//            independently (a quadrant whose pixels all stopped does not wait for the other three), and a quadrant that
//            lies outside the image leaves at once.  The price: the list is staged four times (the four workgroups
//            of a tile are neighbours in the XCD remap, so the repeats can come from one L2).
#include "common.h"
#include "wide_dev.h"

namespace eg {

inline bool tile_size_ok(int ts) { return ts == 8 || ts == 32; }  // (16: binning.hip and the wide entries)

// ---------------------------------------------------------------------------------------------
// compositing
constexpr int kStage8 = 128;   // Gaussians per staging batch, ts = 8 (64 lanes: two per lane)
constexpr int kStage32 = 256;  // ... ts = 16 and 32 (256 threads: one per thread)
constexpr int ts_stage(int ts) { return ts == 8 ? kStage8 : kStage32; }

template <int TS, int CH, bool DEPTH, bool BG>
__global__ void __launch_bounds__(ts_threads(TS))
ts_composite_fwd_kernel(const float4 *__restrict__ splat, const float *__restrict__ colors,
                        const int *__restrict__ offsets, const int *__restrict__ flat, int width, int height, int tw,
                        int th, float *__restrict__ render, float *__restrict__ alphas, int *__restrict__ last_ids,
                        const WideArgs wa) {
  static_assert(CH > 0 || (DEPTH && !BG), "the depth-only form has a depth channel and no background");
  constexpr int THREADS = ts_threads(TS), STAGE = ts_stage(TS), CHA = CH > 0 ? CH : 1;
  __shared__ float4 sA[STAGE];  // x, y, a, b
  __shared__ float4 sB[STAGE];  // c, o, sigma threshold, depth (DEPTH)
  __shared__ __attribute__((aligned(16))) float sC[CH > 0 ? STAGE * CH : 4];

  {
    const int c = blockIdx.y, T = tw * th;
    const size_t hw = (size_t)width * height;
    flat += wide_list_base(offsets, T, c);
    offsets += (size_t)c * (T + 1);
    splat += 2 * (size_t)wa.N * c;
    if (CH > 0 && wa.colors_per_camera) colors += (size_t)wa.N * wa.cs * c;
    render += hw * wa.ps * c;
    if (alphas) alphas += hw * c;
    if (last_ids) last_ids += hw * c;
  }
  int tile, i, j;
  if (!ts_pixel<TS>(tw, th, width, height, tile, i, j)) return;
  const int tid = threadIdx.x;
  const bool inside = (i < height) && (j < width);
  const float px = (float)j + 0.5f, py = (float)i + 0.5f;
  const int start = offsets[tile], end = offsets[tile + 1];

  float T = 1.f;
  float pix[CHA];
#pragma unroll
  for (int k = 0; k < CHA; ++k) pix[k] = 0.f;
  float pix_d = 0.f;
  int last = 0;
  bool done = !inside;

  for (int base = start; base < end; base += STAGE) {
    if (__syncthreads_and(done)) break;
    const int n = min(STAGE, end - base);
    for (int e = tid; e < n; e += THREADS) {
      const int g = flat[base + e];
      const float4 s0 = splat[2 * g], s1 = splat[2 * g + 1];
      sA[e] = s0;
      sB[e] = make_float4(s1.x, s1.y, __logf(255.f * s1.y) + kThrMargin, DEPTH ? s1.z : 0.f);
    }
    if constexpr (CH > 0) stage_colors<CH, THREADS>(sC, colors, flat, base, 1, n, wa);
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
      if constexpr (CH > 0) {
#pragma unroll
        for (int k = 0; k < CH; ++k) pix[k] += sC[t * CH + k] * w;
      }
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
    if constexpr (CH > 0) {
#pragma unroll
      for (int k = 0; k < CH; ++k) {
        if (k < wa.n_real) {
          float v = pix[k];
          if constexpr (BG) v += T * wa.bg[(size_t)blockIdx.y * wa.cs + k];
          out[k] = v;
        }
      }
    }
    if constexpr (DEPTH) out[wa.n_real] = pix_d;  // (the depth channel's background is 0)
  }
}

template <int TS, int CH, bool DEPTH, bool BG>
__global__ void __launch_bounds__(ts_threads(TS))
ts_composite_bwd_kernel(const float4 *__restrict__ splat, const float *__restrict__ colors,
                        const int *__restrict__ offsets, const int *__restrict__ flat, int width, int height, int tw,
                        int th, const float *__restrict__ alphas, const int *__restrict__ last_ids,
                        const float *__restrict__ v_render, const float *__restrict__ v_alphas,
                        float *__restrict__ g2d, float *__restrict__ v_colors, const WideArgs wa) {
  static_assert(CH > 0 || (DEPTH && !BG), "the depth-only form has a depth channel and no background");
  constexpr int THREADS = ts_threads(TS), STAGE = ts_stage(TS), CHA = CH > 0 ? CH : 1;
  __shared__ float4 sA[STAGE];
  __shared__ float4 sB[STAGE];  // c, o, depth (DEPTH), Gaussian id (int bits)
  __shared__ __attribute__((aligned(16))) float sC[CH > 0 ? STAGE * CH : 4];

  {
    const int c = blockIdx.y, T = tw * th;
    const size_t hw = (size_t)width * height, n = (size_t)wa.N;
    flat += wide_list_base(offsets, T, c);
    offsets += (size_t)c * (T + 1);
    splat += 2 * n * c;
    if (CH > 0 && wa.colors_per_camera) colors += n * wa.cs * c;
    alphas += hw * c;
    last_ids += hw * c;
    v_render += hw * wa.ps * c;
    if (v_alphas) v_alphas += hw * c;
    g2d += 8 * n * c;
    if (v_colors) v_colors += n * wa.cs * c;
  }
  int tile, i, j;
  if (!ts_pixel<TS>(tw, th, width, height, tile, i, j)) return;
  const int start = offsets[tile], end = offsets[tile + 1];
  if (end <= start) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const bool inside = (i < height) && (j < width);
  const float px = (float)j + 0.5f, py = (float)i + 0.5f;
  const int p = inside ? i * width + j : 0;

  const float T_final = inside ? 1.f - alphas[p] : 1.f;
  float T = T_final;
  float buffer[CHA], vr[CHA];
#pragma unroll
  for (int k = 0; k < CHA; ++k) {
    buffer[k] = 0.f;
    vr[k] = (CH > 0 && inside && k < wa.n_real) ? v_render[(size_t)p * wa.ps + k] : 0.f;
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

  const int n_batches = (end - start + STAGE - 1) / STAGE;
  for (int b = 0; b < n_batches; ++b) {
    __syncthreads();
    const int batch_end = end - 1 - STAGE * b;
    const int size = min(STAGE, batch_end + 1 - start);
    for (int e = tid; e < size; e += THREADS) {
      const int g = flat[batch_end - e];
      const float4 s0 = splat[2 * g], s1 = splat[2 * g + 1];
      sA[e] = s0;
      sB[e] = make_float4(s1.x, s1.y, DEPTH ? s1.z : 0.f, __int_as_float(g));
    }
    if constexpr (CH > 0) stage_colors<CH, THREADS>(sC, colors, flat, batch_end, -1, size, wa);
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
      float r_rgb[CHA];
#pragma unroll
      for (int k = 0; k < CHA; ++k) r_rgb[k] = 0.f;
      float r_d = 0.f;
      float gv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // g2d record: gx gy |gx| |gy| ga gb gc go
      if (valid) {
        const float ra = 1.f / (1.f - alpha);
        T *= ra;
        const float fac = alpha * T;
        float v_alpha = 0.f;
        if constexpr (CH > 0) {
#pragma unroll
          for (int k = 0; k < CH; ++k) {
            r_rgb[k] = fac * vr[k];
            v_alpha += (sC[t * CH + k] * T - buffer[k] * ra) * vr[k];
          }
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
        if constexpr (CH > 0) {
#pragma unroll
          for (int k = 0; k < CH; ++k) buffer[k] += sC[t * CH + k] * fac;
        }
        if constexpr (DEPTH) buffer_d += B.z * fac;
      }
      const int g = __float_as_int(B.w);
      // component k of the colour sums in lane k (k < CH), of the splat-side sums in lane 32 + k
      float c_sum = 0.f;
      if constexpr (CH > 0) c_sum = lane_transpose_sum<CH>(r_rgb, lane);
      const float g_sum = lane_transpose_sum<8>(gv, lane);
      float *dst = nullptr;
      float val = 0.f;
      if (lane < 32) {
        if (CH > 0 && v_colors && lane < wa.n_real) { dst = v_colors + (size_t)g * wa.cs + lane; val = c_sum; }
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
#define EG_TS_RANGES(C, ranges_host, width, height, tile_size)                                         \
  EG_REQUIRE(tile_size_ok(tile_size), "tile_size must be 8 or 32 (16: eg_tile_count, eg_tile_emit)");   \
  EG_REQUIRE(C >= 1 && C <= 65535 && width > 0 && height > 0, "bad sizes");                            \
  EG_REQUIRE(ranges_host, "null pointer");                                                             \
  EG_REQUIRE(ranges_host[0] >= 0, "bad ranges");                                                       \
  for (int c_ = 0; c_ < C; ++c_)                                                                       \
    EG_REQUIRE(ranges_host[c_ + 1] >= ranges_host[c_] && ranges_host[c_ + 1] - ranges_host[c_] < (1ll << 31), "bad ranges")

extern "C" int eg_tile_count_ts(const float *means2d, const int32_t *radii, const int64_t *ranges_host, int32_t C,
                                int32_t width, int32_t height, int32_t tile_size, int32_t *tiles_per_gauss,
                                int32_t *tile_counts, eg_stream_t stream) {
  EG_TS_RANGES(C, ranges_host, width, height, tile_size);
  if (ranges_host[C] == ranges_host[0]) return EG_OK;
  EG_REQUIRE(means2d && radii && tile_counts, "null pointer");
  const int tw = cdiv(width, tile_size), th = cdiv(height, tile_size);
  const int64_t T = (int64_t)tw * th;
  EG_REQUIRE(T < (1ll << 31), "bad sizes");
  for (int c = 0; c < C; ++c) {
    const int64_t b = ranges_host[c];
    const int n = (int)(ranges_host[c + 1] - b);
    if (n == 0) continue;
    launch_tile_count(means2d + 2 * b, radii + b, n, tile_size, tw, th, tiles_per_gauss ? tiles_per_gauss + b : nullptr,
                      tile_counts + T * c, as_stream(stream));
  }
  return check_launch("tile_count_ts");
}

extern "C" int eg_tile_emit_sort_ts(const float *means2d, const int32_t *radii, const float *depths,
                                    const int64_t *ranges_host, int32_t C, int32_t width, int32_t height,
                                    int32_t tile_size, const int32_t *offsets, int32_t *tile_counts,
                                    const int64_t *M_host, uint64_t *keys, int32_t *flatten_ids, int64_t *isect_ids,
                                    const int32_t *max_tile_host, int32_t rebase, eg_stream_t stream) {
  EG_TS_RANGES(C, ranges_host, width, height, tile_size);
  EG_REQUIRE(offsets && tile_counts && M_host, "null pointer");
  const int tw = cdiv(width, tile_size), th = cdiv(height, tile_size);
  const int64_t T64 = (int64_t)tw * th;
  EG_REQUIRE(T64 < (1ll << 30), "bad sizes");
  const int T = (int)T64;
  const int bits = tile_bits(T);
  for (int c = 0; c < C; ++c) {  // (everything is checked before the first launch)
    const int64_t n = ranges_host[c + 1] - ranges_host[c], M = M_host[c];
    EG_REQUIRE(M >= 0 && (!rebase || ranges_host[c] < (1ll << 31)), "bad sizes");
    EG_REQUIRE(M == 0 || (n > 0 && means2d && radii && depths && keys && flatten_ids), "null pointer");
  }
  int64_t m_base = 0;
  for (int c = 0; c < C; ++c) {
    const int64_t b = ranges_host[c], M = M_host[c];
    const int n = (int)(ranges_host[c + 1] - b);
    if (M > 0) {
      const int rc = bin_camera("tile_emit_sort_ts", means2d + 2 * b, radii + b, depths + b, n, tile_size, tw, th,
                                offsets + (size_t)(T + 1) * c, tile_counts + (size_t)T * c, M, keys + m_base,
                                flatten_ids + m_base, isect_ids ? isect_ids + m_base : nullptr,
                                max_tile_host ? max_tile_host[c] : 0, rebase ? (int)b : 0, (int64_t)c << (32 + bits), stream);
      if (rc) return rc;
    }
    m_base += M;
  }
  return EG_OK;
}

// ---------------------------------------------------------------------------------------------
// Chunked compositing.  Two pairs of entries, each with its own argument checks (the wide pair: 16-pixel tiles, no
// tile_size argument, no depth-only form), then one launcher per direction.
#define EG_WIDE_CHECK(C, N, channels, n_real, depth, width, height, cs, ps)                                  \
  EG_REQUIRE(C >= 1 && C <= 65535 && N >= 0 && width > 0 && height > 0, "bad sizes");                         \
  EG_REQUIRE(channels >= 1 && channels <= 32, "channels (the chunk width) must be 1 .. 32");                  \
  EG_REQUIRE(n_real >= 1 && n_real <= channels, "n_real must be 1 .. channels");                              \
  EG_REQUIRE(cs >= n_real, "color_stride is smaller than the channel count");                                 \
  EG_REQUIRE(ps >= n_real + (depth ? 1 : 0), "pixel_stride is smaller than the channel count")

#define EG_TS_CHECK(C, N, channels, n_real, depth, width, height, tile_size, cs, ps)                          \
  EG_REQUIRE(tile_size_ok(tile_size), "tile_size must be 8 or 32 (16: eg_composite_*_wide_cams)");            \
  EG_REQUIRE(C >= 1 && C <= 65535 && N >= 0 && width > 0 && height > 0, "bad sizes");                         \
  EG_REQUIRE(channels >= 0 && channels <= 32, "channels (the chunk width) must be 0 .. 32");                  \
  EG_REQUIRE(channels > 0 || depth, "channels == 0 (depth only) needs the depth channel");                    \
  EG_REQUIRE(channels > 0 ? (n_real >= 1 && n_real <= channels) : n_real == 0, "n_real must be 1 .. channels"); \
  EG_REQUIRE(channels == 0 || cs >= n_real, "color_stride is smaller than the channel count");                \
  EG_REQUIRE(ps >= n_real + (depth ? 1 : 0), "pixel_stride is smaller than the channel count");               \
  EG_REQUIRE((int64_t)cdiv(width, tile_size) * cdiv(height, tile_size) * 4 < (1ll << 31), "bad sizes")

// tile size, then channel width, then (DEPTH, BG)
#define EG_TS_DB(LAUNCH, TS, CH)                                                        \
  do {                                                                                  \
    if (depth) { if (bg) LAUNCH(TS, CH, true, true); else LAUNCH(TS, CH, true, false); } \
    else { if (bg) LAUNCH(TS, CH, false, true); else LAUNCH(TS, CH, false, false); }     \
  } while (0)

#define EG_TS_CH(LAUNCH, TS)                            \
  do {                                                  \
    if (channels <= 2) EG_TS_DB(LAUNCH, TS, 2);         \
    else if (channels <= 4) EG_TS_DB(LAUNCH, TS, 4);    \
    else if (channels <= 8) EG_TS_DB(LAUNCH, TS, 8);    \
    else if (channels <= 16) EG_TS_DB(LAUNCH, TS, 16);  \
    else EG_TS_DB(LAUNCH, TS, 32);                      \
  } while (0)

// (the depth-only form CH = 0 exists at 8 and 32 alone: at 16 the depth-only modes are composite.hip's)
#define EG_TS_DISPATCH(LAUNCH)                                                                                  \
  do {                                                                                                          \
    if (tile_size == 16) EG_TS_CH(LAUNCH, 16);                                                                  \
    else if (channels == 0) { if (tile_size == 8) LAUNCH(8, 0, true, false); else LAUNCH(32, 0, true, false); } \
    else if (tile_size == 8) EG_TS_CH(LAUNCH, 8);                                                               \
    else EG_TS_CH(LAUNCH, 32);                                                                                  \
  } while (0)

// the colour rows can be fetched in 16-byte (CH = 2: 8-byte) units
static int wide_rows_aligned(const float *colors, int channels, int cs) {
  if (channels == 0) return 0;
  const int vw = channels <= 2 ? 2 : 4;
  return ((uintptr_t)colors % (vw * sizeof(float)) == 0) && (cs % vw == 0);
}

// (the arguments are the entries', checked there; `entry` names the entry in a launch error)
static int ts_composite_fwd_launch(const char *entry, int tile_size, int C, const float *splat, int N,
                                   const float *colors, int colors_per_camera, int channels, int depth,
                                   const float *backgrounds, const int32_t *offsets, const int32_t *flatten_ids,
                                   int width, int height, float *render, float *alphas, int32_t *last_ids, int n_real,
                                   int color_stride, int pixel_stride, eg_stream_t stream) {
  const int tw = cdiv(width, tile_size), th = cdiv(height, tile_size);
  const float *bg = channels > 0 ? backgrounds : nullptr;
  const WideArgs wa = {bg, nullptr, N, colors_per_camera != 0, n_real, color_stride, pixel_stride,
                       wide_rows_aligned(colors, channels, color_stride)};
  hipStream_t s = as_stream(stream);
#define EG_LAUNCH_FWD_TS(TS, CH, DEPTH, BG)                                                                     \
  ts_composite_fwd_kernel<TS, CH, DEPTH, BG><<<dim3(tw * th * ts_sub(TS), C), ts_threads(TS), 0, s>>>(          \
      (const float4 *)splat, colors, offsets, flatten_ids, width, height, tw, th, render, alphas, last_ids, wa)
  EG_TS_DISPATCH(EG_LAUNCH_FWD_TS);
#undef EG_LAUNCH_FWD_TS
  return check_launch(entry);
}

static int ts_composite_bwd_launch(const char *entry, int tile_size, int C, const float *splat, int N,
                                   const float *colors, int colors_per_camera, int channels, int depth,
                                   const float *backgrounds, const int32_t *offsets, const int32_t *flatten_ids,
                                   int width, int height, const float *alphas, const int32_t *last_ids,
                                   const float *v_render, const float *v_alphas, float *g2d, float *v_colors,
                                   float *v_depths, int n_real, int color_stride, int pixel_stride,
                                   eg_stream_t stream) {
  const int tw = cdiv(width, tile_size), th = cdiv(height, tile_size);
  const float *bg = channels > 0 ? backgrounds : nullptr;
  const WideArgs wa = {bg, v_depths, N, colors_per_camera != 0, n_real, color_stride, pixel_stride,
                       wide_rows_aligned(colors, channels, color_stride)};
  hipStream_t s = as_stream(stream);
#define EG_LAUNCH_BWD_TS(TS, CH, DEPTH, BG)                                                                     \
  ts_composite_bwd_kernel<TS, CH, DEPTH, BG><<<dim3(tw * th * ts_sub(TS), C), ts_threads(TS), 0, s>>>(          \
      (const float4 *)splat, colors, offsets, flatten_ids, width, height, tw, th, alphas, last_ids, v_render,      \
      v_alphas, g2d, v_colors, wa)
  EG_TS_DISPATCH(EG_LAUNCH_BWD_TS);
#undef EG_LAUNCH_BWD_TS
  return check_launch(entry);
}
#undef EG_TS_DISPATCH
#undef EG_TS_CH
#undef EG_TS_DB

extern "C" int eg_composite_fwd_wide_cams(int32_t C, const float *splat, int32_t N, const float *colors,
                                          int32_t colors_per_camera, int32_t channels, int32_t depth,
                                          const float *backgrounds, const int32_t *offsets,
                                          const int32_t *flatten_ids, int32_t width, int32_t height, float *render,
                                          float *alphas, int32_t *last_ids, int32_t n_real, int32_t color_stride,
                                          int32_t pixel_stride, eg_stream_t stream) {
  EG_WIDE_CHECK(C, N, channels, n_real, depth, width, height, color_stride, pixel_stride);
  EG_REQUIRE(colors, "null colors (channels > 0)");
  EG_REQUIRE(splat && offsets && flatten_ids && render, "null pointer");
  return ts_composite_fwd_launch("composite_fwd_wide_cams", kTile, C, splat, N, colors, colors_per_camera, channels,
                                 depth, backgrounds, offsets, flatten_ids, width, height, render, alphas, last_ids,
                                 n_real, color_stride, pixel_stride, stream);
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
  return ts_composite_bwd_launch("composite_bwd_wide_cams", kTile, C, splat, N, colors, colors_per_camera, channels,
                                 depth, backgrounds, offsets, flatten_ids, width, height, alphas, last_ids, v_render,
                                 v_alphas, g2d, v_colors, v_depths, n_real, color_stride, pixel_stride, stream);
}

extern "C" int eg_composite_fwd_ts_cams(int32_t C, const float *splat, int32_t N, const float *colors,
                                        int32_t colors_per_camera, int32_t channels, int32_t depth,
                                        const float *backgrounds, const int32_t *offsets, const int32_t *flatten_ids,
                                        int32_t width, int32_t height, int32_t tile_size, float *render, float *alphas,
                                        int32_t *last_ids, int32_t n_real, int32_t color_stride, int32_t pixel_stride,
                                        eg_stream_t stream) {
  EG_TS_CHECK(C, N, channels, n_real, depth, width, height, tile_size, color_stride, pixel_stride);
  EG_REQUIRE(channels == 0 || colors, "null colors (channels > 0)");
  EG_REQUIRE(splat && offsets && flatten_ids && render, "null pointer");
  return ts_composite_fwd_launch("composite_fwd_ts_cams", tile_size, C, splat, N, colors, colors_per_camera, channels,
                                 depth, backgrounds, offsets, flatten_ids, width, height, render, alphas, last_ids,
                                 n_real, color_stride, pixel_stride, stream);
}

extern "C" int eg_composite_bwd_ts_cams(int32_t C, const float *splat, int32_t N, const float *colors,
                                        int32_t colors_per_camera, int32_t channels, int32_t depth,
                                        const float *backgrounds, const int32_t *offsets, const int32_t *flatten_ids,
                                        int32_t width, int32_t height, int32_t tile_size, const float *alphas,
                                        const int32_t *last_ids, const float *v_render, const float *v_alphas,
                                        float *g2d, float *v_colors, float *v_depths, int32_t n_real,
                                        int32_t color_stride, int32_t pixel_stride, eg_stream_t stream) {
  EG_TS_CHECK(C, N, channels, n_real, depth, width, height, tile_size, color_stride, pixel_stride);
  EG_REQUIRE(channels == 0 || colors, "null colors (channels > 0)");
  EG_REQUIRE(splat && offsets && flatten_ids && alphas && last_ids && v_render && g2d, "null pointer");
  EG_REQUIRE(!depth || v_depths, "null v_depths (depth channel)");
  return ts_composite_bwd_launch("composite_bwd_ts_cams", tile_size, C, splat, N, colors, colors_per_camera, channels,
                                 depth, backgrounds, offsets, flatten_ids, width, height, alphas, last_ids, v_render,
                                 v_alphas, g2d, v_colors, v_depths, n_real, color_stride, pixel_stride, stream);
}
#undef EG_TS_CHECK
#undef EG_WIDE_CHECK
#undef EG_TS_RANGES

