// The three operations of gsplat's densification strategies that run on the device every step or every refinement
// (edgegaussians_amd/strategy, edgegaussians_amd/relocation.py).  One lane per Gaussian, 256-thread workgroups, no
// atomics, no LDS, no scratch; contraction off, so every kernel is one fixed fp32 rounding sequence.
//
// eg_compute_relocation: gsplat's `compute_relocation` (the MCMC trainer's opacity / scale correction when a Gaussian
//   is split into r copies).  r = clamp(ratio, 1, n_max), x = 1 - (1 - o)^(1 / r),
//     den = sum_{i = 1..r} sum_{k = 0..i-1} binoms[i-1, k] (-1)^k x^(k+1) / sqrt(k+1)
//   added in fp32 in exactly that order (i outer, k inner, one running sum); new_opacity = x,
//   new_scales = (o / den) scales.  x^(k+1) is a running product restarted at every i (k roundings), 1 / sqrt(k+1) the
//   IEEE square root and division.  The n_max x n_max table (51 x 51 floats = 10 KiB in the MCMC strategy) is read
//   THROUGH THE CACHE, not staged in LDS: its index (i-1) n_max + k does not depend on the lane, so every lane of a
//   wave that is still in the loop reads the same word -- one broadcast line per load, and the whole table stays in the
//   vector L1 -- while an LDS copy would cost every workgroup a 10 KiB fill and a barrier for a call whose N is the
//   number of dead Gaussians (tens to thousands), i.e. a few workgroups that each read only the rows below their largest r.
// eg_inject_noise: MCMC's position noise.  means += Sigma (z * gate * scaler) with Sigma = R diag(s^2) R^T from the
//   rsqrtf-normalised quaternion and s = exp(log_scales) (quat_rot / rdr of csrc/functional.hip, restated here: the six
//   entries are the same bits as quat_scale_to_covar_preci's), gate = 1 / (1 + exp(-100 ((1 - sigmoid(logit)) - 0.995))).
//   56 bytes read, 12 written per Gaussian.
// eg_strategy_update / eg_strategy_update_packed: DefaultStrategy's running statistics.  For every visible pair
//   (radii > 0) of Gaussian n:  grad2d[n] += sqrt((gx sx)^2 + (gy sy)^2), count[n] += 1,
//   radii_state[n] = max(radii_state[n], radii / max_dim).  One lane per Gaussian walks the cameras 0 .. C-1 and adds in
//   that order: the same bits every run, and the same bits in the dense ([C,N,2], [C,N]) and the packed ([nnz,2], [nnz],
//   gaussian_ids, indptr [C+1]) form, which finds its Gaussian in each camera's ascending segment by binary search.
//   Measured at N = 1 M, C = 4 (2.3 M pairs; 0.095 ms with the torch.searchsorted of the segments) and rejected: the
//   searches of four cameras in lock-step in one lane (0.090 ms, within the spread of the runs, for twice the code), and
//   narrowing each segment to the wave's 64 consecutive Gaussians with wave-uniform searches first (0.121 ms).
//   Packed with C == 1: one lane per pair (the ids of one camera are distinct, so no two lanes share a row).
//   PRECONDITION of the packed form, not checked: the pairs are in camera * N + gaussian order (what
//   rasterization(packed=True) returns).  Anything else gives wrong sums -- never an access outside the tensors: segment
//   bounds are clamped to [0, nnz] and every Gaussian id is range-checked before it is used as an index.
#include "common.h"

namespace eg {

constexpr int kSt = 256;  // threads per workgroup of every kernel here

__global__ void __launch_bounds__(kSt)
compute_relocation_kernel(const float *__restrict__ opacities, const float *__restrict__ scales,
                          const int *__restrict__ ratios, const float *__restrict__ binoms, int N, int n_max,
                          float *__restrict__ new_opacities, float *__restrict__ new_scales) {
#pragma clang fp contract(off)
  const int g = blockIdx.x * kSt + threadIdx.x;
  if (g >= N) return;
  const int r = min(max(ratios[g], 1), n_max);
  const float o = opacities[g];
  const float x = 1.f - powf(1.f - o, 1.f / (float)r);
  float den = 0.f;
  for (int i = 1; i <= r; ++i) {
    const float *__restrict__ row = binoms + (size_t)(i - 1) * n_max;
    float xp = x, sign = 1.f;
    for (int k = 0; k < i; ++k) {
      const float term = row[k] * sign * xp / sqrtf((float)(k + 1));
      den = den + term;
      xp = xp * x;
      sign = -sign;
    }
  }
  const float c = o / den;
  new_opacities[g] = x;
  new_scales[3 * (size_t)g] = c * scales[3 * (size_t)g];
  new_scales[3 * (size_t)g + 1] = c * scales[3 * (size_t)g + 1];
  new_scales[3 * (size_t)g + 2] = c * scales[3 * (size_t)g + 2];
}

__global__ void __launch_bounds__(kSt)
inject_noise_kernel(float *__restrict__ means, const float *__restrict__ quats, const float *__restrict__ log_scales,
                    const float *__restrict__ logit_opacities, const float *__restrict__ noise, float scaler, int N) {
#pragma clang fp contract(off)
  const int g = blockIdx.x * kSt + threadIdx.x;
  if (g >= N) return;
  // rotation of the rsqrtf-normalised quaternion (w, x, y, z), as quat_rot of csrc/functional.hip
  float w = quats[4 * (size_t)g], x = quats[4 * (size_t)g + 1], y = quats[4 * (size_t)g + 2], z = quats[4 * (size_t)g + 3];
  const float qinv = rsqrtf(w * w + x * x + y * y + z * z);
  w *= qinv; x *= qinv; y *= qinv; z *= qinv;
  const float x2 = x * x, y2 = y * y, z2 = z * z, xy = x * y, xz = x * z, yz = y * z;
  const float wx = w * x, wy = w * y, wz = w * z;
  const float R[9] = {1.f - 2.f * (y2 + z2), 2.f * (xy - wz),       2.f * (xz + wy),
                      2.f * (xy + wz),       1.f - 2.f * (x2 + z2), 2.f * (yz - wx),
                      2.f * (xz - wy),       2.f * (yz + wx),       1.f - 2.f * (x2 + y2)};
  const float s[3] = {expf(log_scales[3 * (size_t)g]), expf(log_scales[3 * (size_t)g + 1]),
                      expf(log_scales[3 * (size_t)g + 2])};
  // upper triangle (00, 01, 02, 11, 12, 22) of M M^T, M = R diag(s), as rdr of csrc/functional.hip
  float M[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) M[3 * i + k] = R[3 * i + k] * s[k];
  constexpr int ui[6] = {0, 0, 0, 1, 1, 2}, uj[6] = {0, 1, 2, 1, 2, 2};
  float u[6];
#pragma unroll
  for (int e = 0; e < 6; ++e)
    u[e] = M[3 * ui[e]] * M[3 * uj[e]] + M[3 * ui[e] + 1] * M[3 * uj[e] + 1] + M[3 * ui[e] + 2] * M[3 * uj[e] + 2];
  const float opac = 1.f / (1.f + expf(-logit_opacities[g]));
  const float gate = 1.f / (1.f + expf(-100.f * ((1.f - opac) - 0.995f)));
  const float n0 = noise[3 * (size_t)g] * gate * scaler, n1 = noise[3 * (size_t)g + 1] * gate * scaler,
              n2 = noise[3 * (size_t)g + 2] * gate * scaler;
  means[3 * (size_t)g] = means[3 * (size_t)g] + (u[0] * n0 + u[1] * n1 + u[2] * n2);
  means[3 * (size_t)g + 1] = means[3 * (size_t)g + 1] + (u[1] * n0 + u[3] * n1 + u[4] * n2);
  means[3 * (size_t)g + 2] = means[3 * (size_t)g + 2] + (u[2] * n0 + u[4] * n1 + u[5] * n2);
}

struct StatK {
  float sx, sy, max_dim;
};

// one visible pair into the running statistics of its Gaussian (the ONE statement of the arithmetic: all three kernels)
__device__ __forceinline__ void stat_add(float gx, float gy, int radius, const StatK &k, float &sum, float &cnt, float &rmax) {
#pragma clang fp contract(off)
  const float a = gx * k.sx, b = gy * k.sy;
  sum = sum + sqrtf(a * a + b * b);
  cnt = cnt + 1.f;
  rmax = fmaxf(rmax, (float)radius / k.max_dim);
}

__global__ void __launch_bounds__(kSt)
strategy_update_kernel(const float *__restrict__ grads, const int *__restrict__ radii, int C, int N, const StatK k,
                       float *__restrict__ grad2d, float *__restrict__ count, float *__restrict__ radii_state) {
  const int g = blockIdx.x * kSt + threadIdx.x;
  if (g >= N) return;
  float sum = grad2d[g], cnt = count[g], rmax = radii_state ? radii_state[g] : 0.f;
  for (int c = 0; c < C; ++c) {
    const size_t e = (size_t)c * N + g;
    const int rad = radii[e];
    if (rad > 0) stat_add(grads[2 * e], grads[2 * e + 1], rad, k, sum, cnt, rmax);
  }
  grad2d[g] = sum; count[g] = cnt;
  if (radii_state) radii_state[g] = rmax;
}

__global__ void __launch_bounds__(kSt)
strategy_update_packed_kernel(const float *__restrict__ grads, const int *__restrict__ radii,
                              const long long *__restrict__ gaussian_ids, const long long *__restrict__ indptr,
                              long long nnz, int C, int N, const StatK k, float *__restrict__ grad2d,
                              float *__restrict__ count, float *__restrict__ radii_state) {
  const int g = blockIdx.x * kSt + threadIdx.x;
  if (g >= N) return;
  float sum = grad2d[g], cnt = count[g], rmax = radii_state ? radii_state[g] : 0.f;
  for (int c = 0; c < C; ++c) {
    // the camera's segment [lo, hi), clamped into the pair list whatever indptr holds
    long long lo = min(max(indptr[c], 0ll), nnz), hi = min(max(indptr[c + 1], lo), nnz);
    const long long end = hi;
    while (lo < hi) {  // first position with gaussian_ids[pos] >= g; lo <= mid < hi <= nnz
      const long long mid = lo + ((hi - lo) >> 1);
      if (gaussian_ids[mid] < (long long)g) lo = mid + 1; else hi = mid;
    }
    if (lo < end && gaussian_ids[lo] == (long long)g) {
      const int rad = radii[lo];
      if (rad > 0) stat_add(grads[2 * lo], grads[2 * lo + 1], rad, k, sum, cnt, rmax);
    }
  }
  grad2d[g] = sum; count[g] = cnt;
  if (radii_state) radii_state[g] = rmax;
}

// C == 1: one lane per pair; the ids of one camera are distinct (precondition), so every row has one writer
__global__ void __launch_bounds__(kSt)
strategy_update_pairs_kernel(const float *__restrict__ grads, const int *__restrict__ radii,
                             const long long *__restrict__ gaussian_ids, long long nnz, int N, const StatK k,
                             float *__restrict__ grad2d, float *__restrict__ count, float *__restrict__ radii_state) {
  const long long q = (long long)blockIdx.x * kSt + threadIdx.x;
  if (q >= nnz) return;
  const long long g = gaussian_ids[q];
  if (g < 0 || g >= (long long)N) return;
  const int rad = radii[q];
  if (rad <= 0) return;
  float sum = grad2d[g], cnt = count[g], rmax = radii_state ? radii_state[g] : 0.f;
  stat_add(grads[2 * q], grads[2 * q + 1], rad, k, sum, cnt, rmax);
  grad2d[g] = sum; count[g] = cnt;
  if (radii_state) radii_state[g] = rmax;
}

}  // namespace eg

using namespace eg;

extern "C" int eg_compute_relocation(const float *opacities, const float *scales, const int32_t *ratios,
                                     const float *binoms, int32_t N, int32_t n_max, float *new_opacities,
                                     float *new_scales, eg_stream_t stream) {
  EG_REQUIRE(N >= 0, "negative size (N)");
  EG_REQUIRE(n_max >= 1 && n_max <= 4096, "n_max (the side of the binomial table) must be in [1, 4096]");
  EG_REQUIRE(N < (int32_t)((1ll << 31) / 3), "3 N must be below 2^31");
  if (N == 0) return EG_OK;
  EG_REQUIRE(opacities, "opacities is null");
  EG_REQUIRE(scales, "scales is null");
  EG_REQUIRE(ratios, "ratios is null");
  EG_REQUIRE(binoms, "binoms is null");
  EG_REQUIRE(new_opacities, "new_opacities is null");
  EG_REQUIRE(new_scales, "new_scales is null");
  compute_relocation_kernel<<<cdiv(N, kSt), kSt, 0, as_stream(stream)>>>(opacities, scales, ratios, binoms, N, n_max,
                                                                          new_opacities, new_scales);
  return check_launch("compute_relocation");
}

extern "C" int eg_inject_noise(float *means, const float *quats, const float *log_scales, const float *logit_opacities,
                               const float *noise, float scaler, int32_t N, eg_stream_t stream) {
  EG_REQUIRE(N >= 0, "negative size (N)");
  EG_REQUIRE(N < (int32_t)((1ll << 31) / 4), "4 N must be below 2^31");
  if (N == 0) return EG_OK;
  EG_REQUIRE(means, "means is null");
  EG_REQUIRE(quats, "quats is null");
  EG_REQUIRE(log_scales, "log_scales is null");
  EG_REQUIRE(logit_opacities, "logit_opacities is null");
  EG_REQUIRE(noise, "noise is null");
  inject_noise_kernel<<<cdiv(N, kSt), kSt, 0, as_stream(stream)>>>(means, quats, log_scales, logit_opacities, noise,
                                                                    scaler, N);
  return check_launch("inject_noise");
}

static int strategy_sizes_ok(int32_t C, int32_t N, int32_t width, int32_t height) {
  return C >= 1 && N >= 0 && width >= 1 && height >= 1;
}

static StatK make_statk(int32_t C, int32_t width, int32_t height) {
  StatK k;
  k.sx = (float)((double)width / 2.0 * (double)C);
  k.sy = (float)((double)height / 2.0 * (double)C);
  k.max_dim = (float)(width > height ? width : height);
  return k;
}

extern "C" int eg_strategy_update(const float *grads, const int32_t *radii, int32_t C, int32_t N, int32_t width,
                                  int32_t height, float *grad2d, float *count, float *radii_state, eg_stream_t stream) {
  EG_REQUIRE(strategy_sizes_ok(C, N, width, height), "bad size (C >= 1, N >= 0, width >= 1, height >= 1)");
  if (N == 0) return EG_OK;
  EG_REQUIRE(grads, "grads is null");
  EG_REQUIRE(radii, "radii is null");
  EG_REQUIRE(grad2d, "grad2d is null");
  EG_REQUIRE(count, "count is null");
  strategy_update_kernel<<<cdiv(N, kSt), kSt, 0, as_stream(stream)>>>(grads, radii, C, N, make_statk(C, width, height),
                                                                       grad2d, count, radii_state);
  return check_launch("strategy_update");
}

extern "C" int eg_strategy_update_packed(const float *grads, const int32_t *radii, const int64_t *gaussian_ids,
                                         const int64_t *indptr, int64_t nnz, int32_t C, int32_t N, int32_t width,
                                         int32_t height, float *grad2d, float *count, float *radii_state,
                                         eg_stream_t stream) {
  EG_REQUIRE(strategy_sizes_ok(C, N, width, height), "bad size (C >= 1, N >= 0, width >= 1, height >= 1)");
  EG_REQUIRE(nnz >= 0, "negative size (nnz)");
  EG_REQUIRE(nnz < (1ll << 31) * 256, "nnz must be below 2^39");
  if (N == 0 || nnz == 0) return EG_OK;
  EG_REQUIRE(grads, "grads is null");
  EG_REQUIRE(radii, "radii is null");
  EG_REQUIRE(gaussian_ids, "gaussian_ids is null");
  EG_REQUIRE(grad2d, "grad2d is null");
  EG_REQUIRE(count, "count is null");
  const StatK k = make_statk(C, width, height);
  if (C == 1) {
    strategy_update_pairs_kernel<<<cdiv(nnz, kSt), kSt, 0, as_stream(stream)>>>(
        grads, radii, (const long long *)gaussian_ids, (long long)nnz, N, k, grad2d, count, radii_state);
    return check_launch("strategy_update_pairs");
  }
  EG_REQUIRE(indptr, "indptr is null");
  strategy_update_packed_kernel<<<cdiv(N, kSt), kSt, 0, as_stream(stream)>>>(
      grads, radii, (const long long *)gaussian_ids, (const long long *)indptr, (long long)nnz, C, N, k, grad2d, count,
      radii_state);
  return check_launch("strategy_update_packed");
}
