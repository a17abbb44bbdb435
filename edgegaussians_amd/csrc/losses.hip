// Scalar image losses (edgegaussians_amd/losses.py): weighted / masked L1 and L2 of a render against its target, forward
// in two launches (partial sums, finalize), backward in one.
//
//   t_p = w_p |c(x_p) - y_p|^q over the logical [B, C, H, W] problem;  q = 1 or 2;  c = identity or clamp(., 0, 1);
//   w_p = 1, an fp32 weight, or a bool mask read as bytes.  value = (sum_p t_p) / D,  D = 1 (sum), B C H W (mean) or the
//   number of selected elements (mean over a mask, counted as an integer).
//   backward for a cotangent v of the value:
//   g_p = (v / D) w_p q |c(x_p) - y_p|^(q - 1) sign(c(x_p) - y_p) [0 <= x_p <= 1 when clamped],  sign(0) = 0,
//   exactly 0.0 where the mask is false, the weight is 0, the sign is 0 or the clamp gate is shut -- also when D = 0.
//
// Mapping: the logical index p = ((b C + c) H + h) W + w decides everything.  Lane l of workgroup g owns the kQuad
// consecutive indices from (g kThreads + l) kQuad on, whatever the strides are: x, y, w and g are each addressed through
// their own four element strides (0 allowed for y and w: a broadcast operand is an expand), with one 16-byte access per
// quad where the operand's innermost stride is 1, W is a multiple of kQuad and rows and base are 16-byte aligned (4
// bytes for the mask), element by element otherwise.  The arithmetic after the loads is one code path, so both give the
// same bits.
// Reduction: the lane's kQuad terms in index order, the wave's DPP tree, the workgroup's waves in order: one partial
// per workgroup into the caller's slab; the finalize kernel (one wave) adds the slab -- lane l the partials l, l + 64, ..
// in order, then the DPP tree -- and divides by D.  No atomics: the bits do not depend on the run or on the strides.
// Longest addition chain of one term: (kQuad - 1) + 6 + (kThreads / 64 - 1) + (ceil(G / 64) - 1) + 6, G workgroups
// (tests/losses_util.py: depth).  Contraction is off: a term is rounded as written (<= 3 roundings: the difference, the
// square, the weight).
#include "common.h"

using namespace eg;

namespace {

constexpr int kThreads = 256;               // lanes of a workgroup
constexpr int kQuad = 4;                    // consecutive logical indices of a lane
constexpr int kPerWG = kThreads * kQuad;    // logical indices of a workgroup (edgegaussians_amd/losses.py: WG_ELEMS)
constexpr int kFinLanes = 64;               // lanes of the finalize kernel (edgegaussians_amd/losses.py: FIN_LANES)
static_assert(kFinLanes == kWave, "slab_sum_f is one wave");

enum { kWNone = 0, kWFloat = 1, kWMask = 2 };                  // w_kind
enum { kSum = 0, kMean = 1, kMaskMean = 2 };                   // reduction
enum { kVecX = 1, kVecY = 2, kVecW = 4, kVecG = 8 };           // operands that take the 16-byte path

struct Strides {
  int64_t b, c, h, w;
};
struct Shape {
  uint32_t C, H, W, n;  // n = B C H W < 2^31
};
struct Index {
  uint32_t b, c, h, w;
};

__device__ __forceinline__ Index decompose(uint32_t p, const Shape &s) {
  const uint32_t row = p / s.W, plane = row / s.H, b = plane / s.C;
  return {b, plane - b * s.C, row - plane * s.H, p - row * s.W};
}
__device__ __forceinline__ void advance(Index &i, const Shape &s) {
  if (++i.w == s.W) {
    i.w = 0;
    if (++i.h == s.H) {
      i.h = 0;
      if (++i.c == s.C) i.c = 0, ++i.b;
    }
  }
}
__device__ __forceinline__ int64_t offset(const Index &i, const Strides &st) {
  return i.b * st.b + i.c * st.c + i.h * st.h + i.w * st.w;
}

// one aligned access for the quad of an operand on the 16-byte path (4 bytes for the mask)
__device__ __forceinline__ void load_vec(const float *p, float (&out)[kQuad]) {
  const float4 q = *reinterpret_cast<const float4 *>(p);
  out[0] = q.x, out[1] = q.y, out[2] = q.z, out[3] = q.w;
}
__device__ __forceinline__ void load_vec(const uint8_t *p, uint8_t (&out)[kQuad]) {
  const uint32_t q = *reinterpret_cast<const uint32_t *>(p);
#pragma unroll
  for (int k = 0; k < kQuad; ++k) out[k] = (uint8_t)(q >> (8 * k));
}

// the lane's quad of one operand: indices p0 .. p0 + kQuad - 1 (zeros from n on)
template <class T>
__device__ __forceinline__ void load_quad(const T *__restrict__ p, const Strides &st, bool vec, Index i, const Shape &s,
                                          uint32_t p0, T (&out)[kQuad]) {
#pragma unroll
  for (int k = 0; k < kQuad; ++k) out[k] = T(0);
  if (p0 >= s.n) return;
  if (vec) {  // (W % kQuad == 0: the quad lies in one row)
    load_vec(p + offset(i, st), out);
    return;
  }
#pragma unroll
  for (int k = 0; k < kQuad; ++k) {
    if (p0 + k < s.n) out[k] = p[offset(i, st)];
    advance(i, s);
  }
}

__device__ __forceinline__ float residual(float x, float y, int clamp) {
  const float cx = clamp ? (x < 0.f ? 0.f : (x > 1.f ? 1.f : x)) : x;  // (a NaN passes, as through torch.clamp)
  return cx - y;
}

template <int WKIND>
__global__ void __launch_bounds__(kThreads)
loss_fwd_kernel(const float *__restrict__ x, const float *__restrict__ y, const void *__restrict__ w, Shape s, Strides sx,
                Strides sy, Strides sw, int q, int clamp, int vec, float *__restrict__ slab_sum,
                int32_t *__restrict__ slab_count) {
#pragma clang fp contract(off)
  __shared__ float wave_f[kThreads / kWave];
  __shared__ int wave_i[kThreads / kWave];
  const uint32_t p0 = (blockIdx.x * kThreads + threadIdx.x) * kQuad;
  const Index i0 = decompose(p0, s);
  float xs[kQuad], ys[kQuad], wf[kQuad] = {};
  uint8_t wm[kQuad] = {};
  load_quad(x, sx, vec & kVecX, i0, s, p0, xs);
  load_quad(y, sy, vec & kVecY, i0, s, p0, ys);
  if (WKIND == kWFloat) load_quad(static_cast<const float *>(w), sw, vec & kVecW, i0, s, p0, wf);
  if (WKIND == kWMask) load_quad(static_cast<const uint8_t *>(w), sw, vec & kVecW, i0, s, p0, wm);
  float acc = 0.f;
  int count = 0;
#pragma unroll
  for (int k = 0; k < kQuad; ++k) {  // (indices from n on: x = y = 0, a term of 0)
    const float a = fabsf(residual(xs[k], ys[k], clamp));
    float t = q == 2 ? a * a : a;
    if (WKIND == kWFloat) t = wf[k] * t;
    if (WKIND == kWMask) t = wm[k] ? t : 0.f, count += wm[k] != 0;
    acc += t;
  }
  const float total = block_sum_f<kThreads>(acc, wave_f);
  if (threadIdx.x == 0) slab_sum[blockIdx.x] = total;
  if (WKIND == kWMask) {
    const int selected = block_sum_i<kThreads>(count, wave_i);
    if (threadIdx.x == 0) slab_count[blockIdx.x] = selected;
  }
}

// out[0] = sum / D, out[1] = sum, out[2] = D
__global__ void __launch_bounds__(kFinLanes)
loss_finalize_kernel(const float *__restrict__ slab_sum, const int32_t *__restrict__ slab_count, int G, int reduction,
                     float numel, float *__restrict__ out) {
  const float sum = slab_sum_f(slab_sum, G, 1);
  int count = 0;
  if (reduction == kMaskMean) {
    for (int i = threadIdx.x; i < G; i += kFinLanes) count += slab_count[i];
    count = wave_scan_dpp(count, 0, OpAdd());
  }
  if (threadIdx.x == kFinLanes - 1) {
    const float D = reduction == kSum ? 1.f : reduction == kMean ? numel : (float)count;
    out[0] = sum / D, out[1] = sum, out[2] = D;
  }
}

template <int WKIND>
__global__ void __launch_bounds__(kThreads)
loss_bwd_kernel(const float *__restrict__ x, const float *__restrict__ y, const void *__restrict__ w, Shape s, Strides sx,
                Strides sy, Strides sw, Strides sg, int q, int clamp, int vec, const float *__restrict__ v,
                const float *__restrict__ fwd_out, float *__restrict__ g) {
#pragma clang fp contract(off)
  const uint32_t p0 = (blockIdx.x * kThreads + threadIdx.x) * kQuad;
  if (p0 >= s.n) return;
  Index i = decompose(p0, s);
  float xs[kQuad], ys[kQuad], wf[kQuad] = {};
  uint8_t wm[kQuad] = {};
  load_quad(x, sx, vec & kVecX, i, s, p0, xs);
  load_quad(y, sy, vec & kVecY, i, s, p0, ys);
  if (WKIND == kWFloat) load_quad(static_cast<const float *>(w), sw, vec & kVecW, i, s, p0, wf);
  if (WKIND == kWMask) load_quad(static_cast<const uint8_t *>(w), sw, vec & kVecW, i, s, p0, wm);
  const float scale = v[0] / fwd_out[2];  // v / D
  float gs[kQuad];
#pragma unroll
  for (int k = 0; k < kQuad; ++k) {
    const float xv = xs[k], d = residual(xv, ys[k], clamp);
    const float coef = q == 2 ? 2.f * d : (d > 0.f ? 1.f : (d < 0.f ? -1.f : d));
    bool live = (!clamp || (xv >= 0.f && xv <= 1.f)) && coef != 0.f;
    float val = scale * coef;
    if (WKIND == kWFloat) val = (scale * wf[k]) * coef, live = live && wf[k] != 0.f;
    if (WKIND == kWMask) live = live && wm[k];
    gs[k] = live ? val : 0.f;  // (select, not multiply: exactly 0.0 also under scale = inf or nan, D = 0)
  }
  if (vec & kVecG) {
    *reinterpret_cast<float4 *>(g + offset(i, sg)) = make_float4(gs[0], gs[1], gs[2], gs[3]);
    return;
  }
#pragma unroll
  for (int k = 0; k < kQuad; ++k) {
    if (p0 + k < s.n) g[offset(i, sg)] = gs[k];
    advance(i, s);
  }
}

inline int64_t workgroups(int64_t numel) { return (numel + kPerWG - 1) / kPerWG; }
inline Strides strides_of(const int64_t *st) { return {st[0], st[1], st[2], st[3]}; }

// may the operand at `p` take one aligned access of `bytes` per quad?
inline bool quad_aligned(const void *p, const int64_t *st, const int32_t *size, int bytes) {
  if (size[3] % kQuad != 0 || st[3] != 1 || reinterpret_cast<uintptr_t>(p) % bytes != 0) return false;
  for (int i = 0; i < 3; ++i)
    if (size[i] > 1 && st[i] % kQuad != 0) return false;
  return true;
}

// the checks both entries share
#define EG_LOSS_CHECK()                                                                                              \
  do {                                                                                                               \
    EG_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1, "bad sizes (B, C, H, W >= 1)");                                 \
    EG_REQUIRE((int64_t)B * C * H * W < ((int64_t)1 << 31), "B * C * H * W must be below 2^31");                     \
    EG_REQUIRE(x && y, "null x / y");                                                                                \
    EG_REQUIRE(w_kind == kWNone || w_kind == kWFloat || w_kind == kWMask, "w_kind must be 0, 1 or 2");               \
    EG_REQUIRE((w_kind == kWNone) == (w == nullptr), "w: given exactly when w_kind != 0");                           \
    EG_REQUIRE(strides_x && strides_y && (strides_w || w_kind == kWNone), "null strides_x / strides_y / strides_w"); \
    for (int i = 0; i < 4; ++i)                                                                                      \
      EG_REQUIRE(strides_x[i] >= 0 && strides_y[i] >= 0 && (!strides_w || strides_w[i] >= 0), "negative stride");    \
    EG_REQUIRE(q == 1 || q == 2, "q must be 1 or 2");                                                                \
  } while (0)

}  // namespace

extern "C" int eg_loss_fwd(const float *x, const float *y, const void *w, int32_t w_kind, int32_t B, int32_t C, int32_t H,
                           int32_t W, const int64_t *strides_x, const int64_t *strides_y, const int64_t *strides_w,
                           int32_t q, int32_t clamp, int32_t reduction, void *slab, int64_t slab_words, float *out,
                           eg_stream_t stream) {
  EG_LOSS_CHECK();
  EG_REQUIRE(reduction == kSum || reduction == kMean || reduction == kMaskMean, "reduction must be 0, 1 or 2");
  EG_REQUIRE(reduction != kMaskMean || w_kind == kWMask, "the mask mean needs a mask (w_kind 2)");
  const int64_t numel = (int64_t)B * C * H * W;
  const int G = (int)workgroups(numel);
  EG_REQUIRE(slab && out, "null slab / out");
  EG_REQUIRE(slab_words >= (w_kind == kWMask ? 2 : 1) * (int64_t)G, "slab too small (ceil(B C H W / 1024) words, twice with a mask)");
  const int32_t size[4] = {B, C, H, W};
  const int vec = (quad_aligned(x, strides_x, size, 16) ? kVecX : 0) | (quad_aligned(y, strides_y, size, 16) ? kVecY : 0) |
                  (w_kind == kWFloat && quad_aligned(w, strides_w, size, 16) ? kVecW : 0) |
                  (w_kind == kWMask && quad_aligned(w, strides_w, size, 4) ? kVecW : 0);
  const Shape s = {(uint32_t)C, (uint32_t)H, (uint32_t)W, (uint32_t)numel};
  const Strides sx = strides_of(strides_x), sy = strides_of(strides_y), sw = w ? strides_of(strides_w) : Strides{};
  float *slab_sum = static_cast<float *>(slab);
  int32_t *slab_count = w_kind == kWMask ? static_cast<int32_t *>(slab) + G : nullptr;
  hipStream_t st = as_stream(stream);
  if (w_kind == kWNone)
    loss_fwd_kernel<kWNone><<<G, kThreads, 0, st>>>(x, y, w, s, sx, sy, sw, q, clamp != 0, vec, slab_sum, slab_count);
  else if (w_kind == kWFloat)
    loss_fwd_kernel<kWFloat><<<G, kThreads, 0, st>>>(x, y, w, s, sx, sy, sw, q, clamp != 0, vec, slab_sum, slab_count);
  else
    loss_fwd_kernel<kWMask><<<G, kThreads, 0, st>>>(x, y, w, s, sx, sy, sw, q, clamp != 0, vec, slab_sum, slab_count);
  loss_finalize_kernel<<<1, kFinLanes, 0, st>>>(slab_sum, slab_count, G, reduction, (float)numel, out);
  return check_launch("loss_fwd");
}

extern "C" int eg_loss_bwd(const float *x, const float *y, const void *w, int32_t w_kind, int32_t B, int32_t C, int32_t H,
                           int32_t W, const int64_t *strides_x, const int64_t *strides_y, const int64_t *strides_w,
                           int32_t q, int32_t clamp, const float *v, const float *fwd_out, float *g,
                           const int64_t *strides_g, eg_stream_t stream) {
  EG_LOSS_CHECK();
  EG_REQUIRE(v && fwd_out && g, "null v / fwd_out / g");
  EG_REQUIRE(strides_g, "null strides_g");
  const int32_t size[4] = {B, C, H, W};
  for (int i = 0; i < 4; ++i) EG_REQUIRE(strides_g[i] > 0 || (strides_g[i] == 0 && size[i] == 1), "g: a stride below 1");
  const int64_t numel = (int64_t)B * C * H * W;
  const int G = (int)workgroups(numel);
  const int vec = (quad_aligned(x, strides_x, size, 16) ? kVecX : 0) | (quad_aligned(y, strides_y, size, 16) ? kVecY : 0) |
                  (w_kind == kWFloat && quad_aligned(w, strides_w, size, 16) ? kVecW : 0) |
                  (w_kind == kWMask && quad_aligned(w, strides_w, size, 4) ? kVecW : 0) |
                  (quad_aligned(g, strides_g, size, 16) ? kVecG : 0);
  const Shape s = {(uint32_t)C, (uint32_t)H, (uint32_t)W, (uint32_t)numel};
  const Strides sx = strides_of(strides_x), sy = strides_of(strides_y), sw = w ? strides_of(strides_w) : Strides{};
  const Strides sg = strides_of(strides_g);
  hipStream_t st = as_stream(stream);
  if (w_kind == kWNone)
    loss_bwd_kernel<kWNone><<<G, kThreads, 0, st>>>(x, y, w, s, sx, sy, sw, sg, q, clamp != 0, vec, v, fwd_out, g);
  else if (w_kind == kWFloat)
    loss_bwd_kernel<kWFloat><<<G, kThreads, 0, st>>>(x, y, w, s, sx, sy, sw, sg, q, clamp != 0, vec, v, fwd_out, g);
  else
    loss_bwd_kernel<kWMask><<<G, kThreads, 0, st>>>(x, y, w, s, sx, sy, sw, sg, q, clamp != 0, vec, v, fwd_out, g);
  return check_launch("loss_bwd");
}
