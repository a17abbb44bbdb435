// Camera-pose gradient of the projection (gsplat: `fully_fused_projection` backward's v_viewmats [C, 4, 4]).
//
// The projection backwards (project.hip, backward_fused.hip, packed.hip) form the camera-space cotangents of every
// visible pair and keep the Gaussian's share.  The camera's share is a sum over the Gaussians, asked for by pose
// optimisers only: it lives here, in two kernels of its own that nobody else pays for.
//
//   partial  grid (B, C), 256 lanes: one lane per pair of camera blockIdx.y.  A visible pair recomputes forward_geom
//            (open cull limits: it passed the culls in the forward, like the other backwards), runs backward_geom<true>
//            and holds the 12 values of [v_R | v_tr]; every other lane holds zeros.  Sum over the wave with DPP, over
//            the four waves through LDS in wave order, one 12-float partial per workgroup into scratch [C, B, 12].
//   fold     grid (C), 256 lanes: lane t adds the partials t, t + 256, ... in ascending order, then the same
//            wave / four-wave sum; v_viewmats[c] is written whole, the zero bottom row included.
//
// No atomics, a fixed order of additions everywhere: the same inputs give the same bits.  Two layouts: DENSE (pair =
// Gaussian blockIdx.x * 256 + lane, visible when the radius word of the saved [C, N, 8] record is positive) and PACKED
// (pair = indptr[c] + blockIdx.x * 256 + lane inside camera c's range of the packed list, every pair visible).
//
// The covariance form (eg_project_covars_bwd_viewmats): the same two layouts behind forward_geom_covar, the dense one
// told by radii [C, N] (eg_project_covars_fwd_cams_flags has no record).  With cc = Rv S Rv^T, S the world covariance,
// the camera's share of a pair is v_R = v_t mean^T + (v_cc + v_cc^T) Rv S, v_tr = v_t (covar_pair_vjp<true>,
// csrc/covar_dev.h).  The same sums, the same fold kernel.
#include "common.h"
#include "covar_dev.h"
#include "project_dev.h"

namespace eg {

constexpr int kVg = 256;  // lanes per workgroup of both kernels

// the four wave sums of v[0..11] into s_part[wave][0..11], behind a barrier (every lane of the workgroup calls this;
// lanes without a pair hold zeros: the DPP steps read live lanes only)
__device__ __forceinline__ void block_sum12(const float (&v)[12], float (*s_part)[12]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const float r = wave_sum_dpp_f(v[k]);
    if (lane == 63) s_part[wv][k] = r;
  }
  __syncthreads();
}

// CM: the camera model (csrc/project_dev.h), kOrtho with EG_FLAG_ORTHO.
template <bool PACKED, int CM>
__global__ void __launch_bounds__(kVg)
viewmat_partial_kernel(const float *__restrict__ means, const float *__restrict__ quats, const float *__restrict__ scales,
                       const float *__restrict__ opacities, const float *__restrict__ viewmats,
                       const float *__restrict__ Ks, int N, int width, int height, float eps2d, uint32_t flags,
                       const float4 *__restrict__ splat, const long long *__restrict__ indptr, long long nnz,
                       const long long *__restrict__ gaussian_ids, const float4 *__restrict__ g2d,
                       const float *__restrict__ v_comps, const float *__restrict__ v_depths,
                       float *__restrict__ scratch) {
  __shared__ float s_part[kVg / 64][12];
  const int c = blockIdx.y;
  long long p = -1;  // index of the pair in g2d / v_comps / v_depths
  int g = -1;
  if (PACKED) {
    const long long lo = max(0ll, indptr[c]), hi = min(indptr[c + 1], nnz);  // (guards against a caller's stale array)
    const long long q = lo + (long long)blockIdx.x * kVg + threadIdx.x;
    if (q < hi) {
      const long long id = gaussian_ids[q];
      if (id >= 0 && id < N) { p = q; g = (int)id; }
    }
  } else {
    const int i = blockIdx.x * kVg + threadIdx.x;
    if (i < N) {
      const long long q = (long long)c * N + i;
      if (__float_as_int(splat[2 * q + 1].w) > 0) { p = q; g = i; }
    }
  }
  float v[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) v[k] = 0.f;
  if (g >= 0) {
    const Cam cam = load_cam(viewmats + 16 * (size_t)c, Ks + 9 * (size_t)c);
    const Raw raw = load_raw(means, quats, scales, opacities, g);
    const float4 ga = g2d[2 * p], gb = g2d[2 * p + 1];
    Fwd f;
    forward_geom<CM>(cam, raw, width, height, -3.0e38f, 3.0e38f, eps2d, flags, f);
    Grads unused;
    backward_geom<true, CM>(cam, f, eps2d, flags, ga, gb, true, v_comps[p], v_depths ? v_depths[p] : 0.f, unused, v, raw.m);
  }
  block_sum12(v, s_part);
  if (threadIdx.x < 12) {
    const int k = threadIdx.x;
    scratch[((size_t)c * gridDim.x + blockIdx.x) * 12 + k] = ((s_part[0][k] + s_part[1][k]) + s_part[2][k]) + s_part[3][k];
  }
}

// the covariance form of viewmat_partial_kernel: covars [N, 6]; DENSE pairs are visible when radii [C, N] is positive
template <bool PACKED, int CM>
__global__ void __launch_bounds__(kVg)
viewmat_partial_covars_kernel(const float *__restrict__ means, const float *__restrict__ covars,
                              const float *__restrict__ viewmats, const float *__restrict__ Ks, int N, int width,
                              int height, float eps2d, uint32_t flags, const int *__restrict__ radii,
                              const long long *__restrict__ indptr, long long nnz,
                              const long long *__restrict__ gaussian_ids, const float4 *__restrict__ g2d,
                              const float *__restrict__ v_comps, const float *__restrict__ v_depths,
                              float *__restrict__ scratch) {
  __shared__ float s_part[kVg / 64][12];
  const int c = blockIdx.y;
  long long p = -1;  // index of the pair in g2d / v_comps / v_depths
  int g = -1;
  if (PACKED) {
    const long long lo = max(0ll, indptr[c]), hi = min(indptr[c + 1], nnz);  // (guards against a caller's stale array)
    const long long q = lo + (long long)blockIdx.x * kVg + threadIdx.x;
    if (q < hi) {
      const long long id = gaussian_ids[q];
      if (id >= 0 && id < N) { p = q; g = (int)id; }
    }
  } else {
    const int i = blockIdx.x * kVg + threadIdx.x;
    if (i < N) {
      const long long q = (long long)c * N + i;
      if (radii[q] > 0) { p = q; g = i; }
    }
  }
  float v[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) v[k] = 0.f;
  if (g >= 0) {
    const Cam cam = load_cam(viewmats + 16 * (size_t)c, Ks + 9 * (size_t)c);
    float m[3], cv[6], cc[6], q0[3], q1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) m[k] = means[3 * (size_t)g + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) cv[k] = covars[6 * (size_t)g + k];
    Fwd f;
    // open cull limits: the pair passed the culls in the forward (a det cull here leaves the lane's zeros)
    if (forward_geom_covar<CM>(cam, m, cv, width, height, -3.0e38f, 3.0e38f, eps2d, f, cc, q0, q1)) {
      const CovarCot ct = load_covar_cot(g2d, v_comps, v_depths, p, flags & EG_FLAG_ANTIALIASED);
      covar_pair_vjp<true, CM>(cam, m, cv, f, q0, q1, eps2d, ct, nullptr, nullptr, v);
    }
  }
  block_sum12(v, s_part);
  if (threadIdx.x < 12) {
    const int k = threadIdx.x;
    scratch[((size_t)c * gridDim.x + blockIdx.x) * 12 + k] = ((s_part[0][k] + s_part[1][k]) + s_part[2][k]) + s_part[3][k];
  }
}

__global__ void __launch_bounds__(kVg)
viewmat_fold_kernel(const float *__restrict__ scratch, int B, float *__restrict__ v_viewmats) {
  __shared__ float s_part[kVg / 64][12];
  const int c = blockIdx.x;
  float v[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) v[k] = 0.f;
  for (int b = threadIdx.x; b < B; b += kVg) {
    const float *part = scratch + ((size_t)c * B + b) * 12;
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] += part[k];
  }
  block_sum12(v, s_part);
  if (threadIdx.x < 16) {
    const int k = threadIdx.x;
    v_viewmats[16 * (size_t)c + k] = k < 12 ? ((s_part[0][k] + s_part[1][k]) + s_part[2][k]) + s_part[3][k] : 0.f;
  }
}

}  // namespace eg

using namespace eg;

extern "C" int eg_project_bwd_viewmats(const float *means, const float *quats, const float *scales,
                                       const float *opacities, const float *viewmats, const float *Ks, int32_t N,
                                       int32_t C, int32_t width, int32_t height, float eps2d, uint32_t flags,
                                       const float *splat, const int64_t *indptr, int64_t nnz,
                                       const int64_t *gaussian_ids, const float *g2d, const float *v_comps,
                                       const float *v_depths, float *scratch, int32_t scratch_blocks,
                                       float *v_viewmats, eg_stream_t stream) {
  EG_REQUIRE(N >= 0 && C >= 1 && C <= 65535 && width > 0 && height > 0, "bad sizes");
  EG_REQUIRE(nnz >= 0 && nnz <= (int64_t)N * C, "bad nnz");
  EG_REQUIRE(viewmats && Ks && v_viewmats, "null pointer");
  const bool packed = splat == nullptr;
  EG_REQUIRE(packed ? (indptr != nullptr) : (nnz == 0 && !indptr && !gaussian_ids), "dense record or packed lists, not both");
  const int B = cdiv(packed ? (nnz < N ? nnz : (int64_t)N) : (int64_t)N, kVg);  // (a camera owns at most min(nnz, N) pairs)
  EG_REQUIRE(scratch_blocks >= B, "scratch too small");
  if (B > 0) {
    EG_REQUIRE(means && quats && scales && opacities && g2d && v_comps && scratch, "null pointer");
    EG_REQUIRE(!packed || gaussian_ids, "null pointer");
  }
  hipStream_t s = as_stream(stream);
#define EG_VIEWMAT_PARTIAL(PACKED_, CM_)                                                                             \
  viewmat_partial_kernel<PACKED_, CM_><<<dim3(B, C), kVg, 0, s>>>(                                                   \
      means, quats, scales, opacities, viewmats, Ks, N, width, height, eps2d, flags, (const float4 *)splat,          \
      (const long long *)indptr, (long long)nnz, (const long long *)gaussian_ids, (const float4 *)g2d, v_comps,      \
      v_depths, scratch)
  if (B > 0) {  // (dense: indptr, nnz and gaussian_ids are NULL / 0, checked above; packed: splat is NULL)
    if (flags & EG_FLAG_ORTHO) {
      if (packed) EG_VIEWMAT_PARTIAL(true, kOrtho); else EG_VIEWMAT_PARTIAL(false, kOrtho);
    } else {
      if (packed) EG_VIEWMAT_PARTIAL(true, kPinhole); else EG_VIEWMAT_PARTIAL(false, kPinhole);
    }
  }
#undef EG_VIEWMAT_PARTIAL
  viewmat_fold_kernel<<<C, kVg, 0, s>>>(scratch, B, v_viewmats);
  return check_launch("project_bwd_viewmats");
}

// the covariance form: covars [N, 6] in place of quats + scales, radii [C, N] in place of the dense record
extern "C" int eg_project_covars_bwd_viewmats(const float *means, const float *covars, const float *viewmats,
                                              const float *Ks, int32_t N, int32_t C, int32_t width, int32_t height,
                                              float eps2d, uint32_t flags, const int32_t *radii, const int64_t *indptr,
                                              int64_t nnz, const int64_t *gaussian_ids, const float *g2d,
                                              const float *v_comps, const float *v_depths, float *scratch,
                                              int32_t scratch_blocks, float *v_viewmats, eg_stream_t stream) {
  EG_REQUIRE(N >= 0 && C >= 1 && C <= 65535 && width > 0 && height > 0, "bad sizes");
  EG_REQUIRE(nnz >= 0 && nnz <= (int64_t)N * C, "bad nnz");
  EG_REQUIRE(viewmats && Ks && v_viewmats, "null pointer");
  const bool packed = radii == nullptr;
  EG_REQUIRE(packed ? (indptr != nullptr) : (nnz == 0 && !indptr && !gaussian_ids), "dense radii or packed lists, not both");
  const int B = cdiv(packed ? (nnz < N ? nnz : (int64_t)N) : (int64_t)N, kVg);  // (a camera owns at most min(nnz, N) pairs)
  EG_REQUIRE(scratch_blocks >= B, "scratch too small");
  if (B > 0) {
    EG_REQUIRE(means && covars && g2d && scratch, "null pointer");
    EG_REQUIRE(!(flags & EG_FLAG_ANTIALIASED) || v_comps, "null pointer");
    EG_REQUIRE(!packed || gaussian_ids, "null pointer");
  }
  hipStream_t s = as_stream(stream);
#define EG_VIEWMAT_PARTIAL(PACKED_, CM_)                                                                             \
  viewmat_partial_covars_kernel<PACKED_, CM_><<<dim3(B, C), kVg, 0, s>>>(                                            \
      means, covars, viewmats, Ks, N, width, height, eps2d, flags, radii, (const long long *)indptr, (long long)nnz, \
      (const long long *)gaussian_ids, (const float4 *)g2d, v_comps, v_depths, scratch)
  if (B > 0) {  // (dense: indptr, nnz and gaussian_ids are NULL / 0, checked above; packed: radii is NULL)
    if (flags & EG_FLAG_ORTHO) {
      if (packed) EG_VIEWMAT_PARTIAL(true, kOrtho); else EG_VIEWMAT_PARTIAL(false, kOrtho);
    } else {
      if (packed) EG_VIEWMAT_PARTIAL(true, kPinhole); else EG_VIEWMAT_PARTIAL(false, kPinhole);
    }
  }
#undef EG_VIEWMAT_PARTIAL
  viewmat_fold_kernel<<<C, kVg, 0, s>>>(scratch, B, v_viewmats);
  return check_launch("project_covars_bwd_viewmats");
}
