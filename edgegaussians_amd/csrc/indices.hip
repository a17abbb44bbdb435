// Per-pixel intersection lists (gsplat rasterize_to_indices_in_range / accumulate; edgegaussians_amd/functional.py).
//
// indices_kernel<TS, WRITE>: the forward walk of the chunked compositing kernels (tiles.hip) -- the same
// source expressions for sigma, the threshold skip, alpha, the 1/255 cut and the transmittance stop, compiled with the
// same flags -- over the batches [range_start, range_end) of every tile's list, a batch being TS * TS LIST ENTRIES,
// starting from a caller's transmittance per pixel.  It does not composite; it COUNTS the entries a pixel takes
// (WRITE = false: counts [C H W]) or WRITES them (WRITE = true: the caller has scanned the counts into 64-bit starts,
// and the pixel's rows are [starts[p], starts[p] + count)).  Two passes of one deterministic walk, no atomics: the
// rows come out in (camera, pixel) order and in list order inside a pixel, the same bits every run.
//
// Workgroup shapes and pixel mapping are the compositing's (ts_pixel, wide_dev.h): TS = 8 one 64-lane workgroup per
// tile, TS = 16 one 256-thread workgroup per tile, TS = 32 one 256-thread workgroup per 16 x 16 quadrant.  A round
// stages kIxStage = 64 (TS = 8) or 256 entries through LDS: two float4 per entry, 2 / 8 KiB per workgroup, far below what would bound the occupancy (8 workgroups of
// four waves fill a CU's 32 wave slots at 64 KiB of its 160 KiB); the stage divides the batch, so the range bounds
// fall on round boundaries.  Every thread reaches every barrier: a thread whose pixel lies outside the image stages
// with the others and is "done" from the start, the loop bounds depend on the tile alone, and the only break is
// __syncthreads_and(done).
//
// Bounds.  A tile's range is the camera's list base plus its local offsets, clamped into [0, n_isects] with end >=
// start before anything is loaded, so no offsets can send a load outside flatten_ids; the ids themselves are the
// caller's (flatten_id mod N, in [0, N)).  A row is stored only below `total`.
//
// accumulate_{fwd,bwd}_kernel<CH>: the segmented product and sum of gsplat's `accumulate` for one chunk of up to 32
// channels: lane p owns pixel p's segment [starts[p], starts[p] + counts[p]) of the entry arrays (clamped into [0, M]),
// so nothing is shared between lanes and nothing is atomic.  The forward leaves T_k, the transmittance in front of
// entry k; the backward walks the segment in reverse with the suffix recurrence  S <- alpha s + (1 - alpha) S,
// s = feat . v_render + v_alphas,  v_alpha = T_k (s - S),  v_feat = alpha T_k v_render -- no division by (1 - alpha).
// Both are linear in the channels, so a wide D is a sequence of chunk launches: the first writes alphas / T_k / v_alpha
// (and carries v_alphas), the later ones add their channels' share to v_alpha.
#include "common.h"
#include "wide_dev.h"

namespace eg {

constexpr int ix_stage(int ts) { return ts == 8 ? 64 : 256; }  // entries per staging round; divides ts * ts

template <int TS, bool WRITE>
__global__ void __launch_bounds__(ts_threads(TS))
indices_kernel(const float2 *__restrict__ means2d, const float *__restrict__ conics,
               const float *__restrict__ opacities, const float *__restrict__ transmittances,
               const int *__restrict__ offsets, const int *__restrict__ flat, long long n_isects, int N, int width,
               int height, int tw, int th, long long range_start, long long range_end, int *__restrict__ counts,
               const long long *__restrict__ starts, long long total, long long *__restrict__ gaussian_ids,
               long long *__restrict__ pixel_ids, long long *__restrict__ camera_ids) {
  constexpr int THREADS = ts_threads(TS), STAGE = ix_stage(TS);
  constexpr long long BATCH = (long long)TS * TS;
  static_assert(BATCH % STAGE == 0 && STAGE <= THREADS, "a round is one entry per thread and divides the batch");
  __shared__ float4 sA[STAGE];  // x, y, a, b
  __shared__ float4 sB[STAGE];  // c, o, sigma threshold, Gaussian id (int bits)

  const int c = blockIdx.y, n_tiles = tw * th, tid = threadIdx.x;
  int tile, i, j;
  if (!ts_pixel<TS>(tw, th, width, height, tile, i, j)) return;  // (a quadrant outside the image: the whole workgroup)

  // the tile's entries [lo, hi) of flat, then the call's batches of them [first, last): workgroup-uniform
  long long lo = 0;
  for (int k = 0; k < c; ++k) lo += offsets[(size_t)k * (n_tiles + 1) + n_tiles];
  offsets += (size_t)c * (n_tiles + 1);
  long long hi = lo + offsets[tile + 1];
  lo += offsets[tile];
  lo = min(max(lo, 0ll), n_isects);
  hi = min(max(hi, lo), n_isects);
  const long long first = min(hi, lo + range_start * BATCH);  // (range_start, range_end <= 2^31: no overflow)
  const long long last = min(hi, lo + range_end * BATCH);

  const bool inside = (i < height) && (j < width);
  const float px = (float)j + 0.5f, py = (float)i + 0.5f;
  const int p = i * width + j;
  const size_t pix = (size_t)c * width * height + (inside ? p : 0);
  const size_t rec = (size_t)c * N;

  float T = inside ? transmittances[pix] : 0.f;
  bool done = !inside;
  int taken = 0;
  long long out = 0;
  if constexpr (WRITE) out = inside ? starts[pix] : 0;

  for (long long base = first; base < last; base += STAGE) {
    if (__syncthreads_and(done)) break;
    const int n = (int)min((long long)STAGE, last - base);
    if (tid < n) {
      const int g = flat[base + tid];
      const float2 m = means2d[rec + g];
      const float *con = conics + 3 * (rec + g);
      const float o = opacities[rec + g];
      sA[tid] = make_float4(m.x, m.y, con[0], con[1]);
      sB[tid] = make_float4(con[2], o, __logf(255.f * o) + kThrMargin, __int_as_float(g));
    }
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
      if constexpr (WRITE) {
        const long long k = out + taken;
        if (k >= 0 && k < total) {
          gaussian_ids[k] = __float_as_int(B.w);
          pixel_ids[k] = p;
          camera_ids[k] = c;
        }
      }
      ++taken;
      T = next_T;
    }
  }
  if constexpr (!WRITE) {
    if (inside) counts[pix] = taken;
  }
}

// one pixel's segment of the M entries
__device__ __forceinline__ void segment_of(const long long *__restrict__ starts, const long long *__restrict__ counts,
                                           long long p, long long M, long long &s, long long &e) {
  s = min(max(starts[p], 0ll), M);
  e = s + min(max(counts[p], 0ll), M - s);
}

template <int CH>
__global__ void __launch_bounds__(256)
accumulate_fwd_kernel(const float *__restrict__ alpha, const float *__restrict__ feat, int fs, int n_real,
                      const long long *__restrict__ starts, const long long *__restrict__ counts, long long P,
                      long long M, float *__restrict__ render, int ps, float *__restrict__ alphas,
                      float *__restrict__ Tk) {
  const long long p = blockIdx.x * 256ll + threadIdx.x;
  if (p >= P) return;
  long long s, e;
  segment_of(starts, counts, p, M, s, e);
  float T = 1.f, wsum = 0.f;
  float acc[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) acc[k] = 0.f;
  for (long long k = s; k < e; ++k) {
    const float a = alpha[k];
    const float w = a * T;
    if (Tk) Tk[k] = T;
    const float *row = feat + (size_t)k * fs;
#pragma unroll
    for (int ch = 0; ch < CH; ++ch)
      if (ch < n_real) acc[ch] += row[ch] * w;
    wsum += w;
    T *= 1.f - a;
  }
  float *dst = render + (size_t)p * ps;
#pragma unroll
  for (int ch = 0; ch < CH; ++ch)
    if (ch < n_real) dst[ch] = acc[ch];
  if (alphas) alphas[p] = wsum;
}

template <int CH>
__global__ void __launch_bounds__(256)
accumulate_bwd_kernel(const float *__restrict__ alpha, const float *__restrict__ feat, int fs, int n_real,
                      const long long *__restrict__ starts, const long long *__restrict__ counts, long long P,
                      long long M, const float *__restrict__ Tk, const float *__restrict__ v_render, int ps,
                      const float *__restrict__ v_alphas, float *__restrict__ v_alpha, int add,
                      float *__restrict__ v_feat) {
  const long long p = blockIdx.x * 256ll + threadIdx.x;
  if (p >= P) return;
  long long s, e;
  segment_of(starts, counts, p, M, s, e);
  float vr[CH];
#pragma unroll
  for (int ch = 0; ch < CH; ++ch) vr[ch] = ch < n_real ? v_render[(size_t)p * ps + ch] : 0.f;
  const float va = v_alphas ? v_alphas[p] : 0.f;
  float S = 0.f;  // sum over the entries behind k of alpha_j s_j prod_{k < k' < j} (1 - alpha_k')
  for (long long k = e - 1; k >= s; --k) {
    const float a = alpha[k], T = Tk[k];
    const float *row = feat + (size_t)k * fs;
    float *vrow = v_feat + (size_t)k * fs;
    const float fac = a * T;
    float sk = va;
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
      if (ch < n_real) {
        sk += row[ch] * vr[ch];
        vrow[ch] = fac * vr[ch];
      }
    }
    const float g = T * (sk - S);
    v_alpha[k] = add ? v_alpha[k] + g : g;
    S = a * sk + (1.f - a) * S;
  }
}

}  // namespace eg

using namespace eg;

#define EG_IX_CHECK(C, N, width, height, tile_size, range_start, range_end)                                   \
  EG_REQUIRE(tile_size == 8 || tile_size == 16 || tile_size == 32, "tile_size must be 8, 16 or 32");          \
  EG_REQUIRE(C >= 0 && C <= 65535 && N >= 0 && width >= 0 && height >= 0 && n_isects >= 0, "bad sizes");      \
  EG_REQUIRE(range_start >= 0 && range_end >= 0, "bad range");                                                \
  EG_REQUIRE((int64_t)cdiv(width, tile_size) * cdiv(height, tile_size) * 4 < (1ll << 31), "bad sizes")

#define EG_IX_DISPATCH(WRITE)                                                                                        \
  do {                                                                                                               \
    const int tw = cdiv(width, tile_size), th = cdiv(height, tile_size);                                             \
    hipStream_t s = as_stream(stream);                                                                               \
    if (tile_size == 8) EG_IX_LAUNCH(8, WRITE); else if (tile_size == 16) EG_IX_LAUNCH(16, WRITE);                   \
    else EG_IX_LAUNCH(32, WRITE);                                                                                    \
  } while (0)

#define EG_IX_LAUNCH(TS, WRITE)                                                                                      \
  indices_kernel<TS, WRITE><<<dim3(tw * th * ts_sub(TS), C), ts_threads(TS), 0, s>>>(                                \
      (const float2 *)means2d, conics, opacities, transmittances, offsets, flatten_ids, (long long)n_isects, N, width, \
      height, tw, th, (long long)range_start, (long long)range_end, counts_, starts_, (long long)total_,              \
      (long long *)gids_, (long long *)pids_, (long long *)cids_)

extern "C" int eg_indices_count(int32_t C, int32_t N, const float *means2d, const float *conics,
                                const float *opacities, const float *transmittances, const int32_t *offsets,
                                const int32_t *flatten_ids, int64_t n_isects, int32_t width, int32_t height,
                                int32_t tile_size, int32_t range_start, int32_t range_end, int32_t *counts,
                                eg_stream_t stream) {
  EG_IX_CHECK(C, N, width, height, tile_size, range_start, range_end);
  EG_REQUIRE(means2d && conics && opacities && transmittances && offsets && flatten_ids && counts, "null pointer");
  if ((int64_t)C * width * height == 0 || N == 0) return EG_OK;
  int32_t *counts_ = counts;
  const long long *starts_ = nullptr;
  const int64_t total_ = 0;
  int64_t *gids_ = nullptr, *pids_ = nullptr, *cids_ = nullptr;
  EG_IX_DISPATCH(false);
  return check_launch("indices_count");
}

extern "C" int eg_indices_write(int32_t C, int32_t N, const float *means2d, const float *conics,
                                const float *opacities, const float *transmittances, const int32_t *offsets,
                                const int32_t *flatten_ids, int64_t n_isects, int32_t width, int32_t height,
                                int32_t tile_size, int32_t range_start, int32_t range_end, const int64_t *starts,
                                int64_t total, int64_t *gaussian_ids, int64_t *pixel_ids, int64_t *camera_ids,
                                eg_stream_t stream) {
  EG_IX_CHECK(C, N, width, height, tile_size, range_start, range_end);
  EG_REQUIRE(total >= 0, "bad sizes");
  EG_REQUIRE(means2d && conics && opacities && transmittances && offsets && flatten_ids && starts && gaussian_ids &&
                 pixel_ids && camera_ids, "null pointer");
  if ((int64_t)C * width * height == 0 || N == 0) return EG_OK;
  int32_t *counts_ = nullptr;
  const long long *starts_ = (const long long *)starts;
  const int64_t total_ = total;
  int64_t *gids_ = gaussian_ids, *pids_ = pixel_ids, *cids_ = camera_ids;
  EG_IX_DISPATCH(true);
  return check_launch("indices_write");
}
#undef EG_IX_LAUNCH
#undef EG_IX_DISPATCH
#undef EG_IX_CHECK

#define EG_ACC_CHECK(channels, feat_stride, pixel_stride, P, M)                                            \
  EG_REQUIRE(channels >= 1 && channels <= 32, "channels (the chunk width) must be 1 .. 32");                \
  EG_REQUIRE(feat_stride >= channels && pixel_stride >= channels, "a stride is smaller than the channel count"); \
  EG_REQUIRE(P >= 0 && M >= 0 && (P + 255) / 256 < (1ll << 31), "bad sizes")

#define EG_ACC_DISPATCH(LAUNCH)             \
  do {                                      \
    if (channels <= 1) LAUNCH(1);           \
    else if (channels <= 2) LAUNCH(2);      \
    else if (channels <= 4) LAUNCH(4);      \
    else if (channels <= 8) LAUNCH(8);      \
    else if (channels <= 16) LAUNCH(16);    \
    else LAUNCH(32);                        \
  } while (0)

extern "C" int eg_accumulate_fwd(const float *alpha, const float *feat, int32_t feat_stride, int32_t channels,
                                 const int64_t *starts, const int64_t *counts, int64_t P, int64_t M, float *render,
                                 int32_t pixel_stride, float *alphas, float *T_k, eg_stream_t stream) {
  EG_ACC_CHECK(channels, feat_stride, pixel_stride, P, M);
  EG_REQUIRE(alpha && feat && starts && counts && render, "null pointer");
  if (P == 0) return EG_OK;
  hipStream_t s = as_stream(stream);
#define EG_LAUNCH_ACC_FWD(CH)                                                                                    \
  accumulate_fwd_kernel<CH><<<(unsigned)((P + 255) / 256), 256, 0, s>>>(                                         \
      alpha, feat, feat_stride, channels, (const long long *)starts, (const long long *)counts, (long long)P,    \
      (long long)M, render, pixel_stride, alphas, T_k)
  EG_ACC_DISPATCH(EG_LAUNCH_ACC_FWD);
#undef EG_LAUNCH_ACC_FWD
  return check_launch("accumulate_fwd");
}

extern "C" int eg_accumulate_bwd(const float *alpha, const float *feat, int32_t feat_stride, int32_t channels,
                                 const int64_t *starts, const int64_t *counts, int64_t P, int64_t M, const float *T_k,
                                 const float *v_render, int32_t pixel_stride, const float *v_alphas, float *v_alpha,
                                 int32_t add, float *v_feat, eg_stream_t stream) {
  EG_ACC_CHECK(channels, feat_stride, pixel_stride, P, M);
  EG_REQUIRE(alpha && feat && starts && counts && T_k && v_render && v_alpha && v_feat, "null pointer");
  if (P == 0) return EG_OK;
  hipStream_t s = as_stream(stream);
#define EG_LAUNCH_ACC_BWD(CH)                                                                                    \
  accumulate_bwd_kernel<CH><<<(unsigned)((P + 255) / 256), 256, 0, s>>>(                                         \
      alpha, feat, feat_stride, channels, (const long long *)starts, (const long long *)counts, (long long)P,    \
      (long long)M, T_k, v_render, pixel_stride, v_alphas, v_alpha, add, v_feat)
  EG_ACC_DISPATCH(EG_LAUNCH_ACC_BWD);
#undef EG_LAUNCH_ACC_BWD
  return check_launch("accumulate_bwd");
}
#undef EG_ACC_DISPATCH
#undef EG_ACC_CHECK
