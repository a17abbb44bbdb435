// Camera-pose gradient of the projection (gsplat: `fully_fused_projection` backward's v_viewmats [C, 4, 4]).
//
// The projection backwards (project.hip, backward_fused.hip, packed.hip) form the camera-space cotangents of every
// visible pair and keep the Gaussian's share.  The camera's share is a sum over the Gaussians, asked for by pose
// optimisers only: it lives here, in two kernels of its own that nobody else pays for.
//
//   partial  grid (B, C), 256 lanes: one lane per pair of camera blockIdx.y.  A visible pair recomputes its forward
//            (open cull limits: it passed the culls in the forward, like the other backwards), runs the reverse sweep
//            up to the camera (quats + scales: backward_geom<true>) and holds the 12 values of [v_R | v_tr]; every
//            other lane holds zeros.  Sum over the wave with DPP, over the four waves through LDS in wave order, one
//            12-float partial per workgroup into scratch [C, B, 12].
//   fold     grid (C), 256 lanes: lane t adds the partials t, t + 256, ... in ascending order, then the same
//            wave / four-wave sum; v_viewmats[c] is written whole, the zero bottom row included.
//
// No atomics, a fixed order of additions everywhere: the same inputs give the same bits.  Two layouts: DENSE (pair =
// Gaussian blockIdx.x * 256 + lane, visible when the radius word of the saved [C, N, 8] record is positive) and PACKED
// (pair = indptr[c] + blockIdx.x * 256 + lane inside camera c's range of the packed list, every pair visible).
//
// The partial kernel is a template over the form the Gaussian's shape arrives in (QuatScaleForm, csrc/project_dev.h;
// CovarForm, csrc/covar_dev.h, behind eg_project_covars_bwd_viewmats): the form's pair_vjp<true> leaves the camera's
// share of a pair, and the form tells which DENSE pairs are visible -- the radius word of the record, or radii [C, N]
// (eg_project_covars_fwd_cams_flags has no record).  With cc = Rv S Rv^T, S the world covariance, the covariance form's
// share is v_R = v_t mean^T + (v_cc + v_cc^T) Rv S, v_tr = v_t (covar_pair_vjp<true>).  The same sums, the same fold.
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

// CM: the camera model (csrc/project_dev.h), kOrtho with EG_FLAG_ORTHO.  `vis`: what Form::visible reads (DENSE only).
template <class Form, bool PACKED, int CM>
__global__ void __launch_bounds__(kVg)
viewmat_partial_kernel(Form form, const float *__restrict__ viewmats, const float *__restrict__ Ks, int N, int width,
                       int height, float eps2d, uint32_t flags, const typename Form::Visible *__restrict__ vis,
                       const long long *__restrict__ indptr, long long nnz, const long long *__restrict__ gaussian_ids,
                       const float4 *__restrict__ g2d, const float *__restrict__ v_comps,
                       const float *__restrict__ v_depths, float *__restrict__ scratch) {
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
      if (Form::visible(vis, q)) { p = q; g = i; }
    }
  }
  float v[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) v[k] = 0.f;
  if (g >= 0) {
    const Cam cam = load_cam(viewmats + 16 * (size_t)c, Ks + 9 * (size_t)c);
    typename Form::Grad unused;
    form.template pair_vjp<true, CM>(cam, g, p, width, height, eps2d, flags, g2d, v_comps, v_depths, unused, v);
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

// the B partials of every camera (dense: `vis`, and indptr, nnz and gaussian_ids are NULL / 0; packed: vis is NULL --
// the entries check that), then the fold
template <class Form>
static void launch_viewmats(const Form &form, const float *viewmats, const float *Ks, int N, int C, int width, int height,
                            float eps2d, uint32_t flags, const typename Form::Visible *vis, const int64_t *indptr,
                            int64_t nnz, const int64_t *gaussian_ids, const float *g2d, const float *v_comps,
                            const float *v_depths, float *scratch, int B, float *v_viewmats, hipStream_t s) {
  if (B > 0)
    with_cam_model(flags, [&](auto cm) {
      constexpr int CM = decltype(cm)::value;
      auto launch = [&](auto kernel) {
        kernel<<<dim3(B, C), kVg, 0, s>>>(form, viewmats, Ks, N, width, height, eps2d, flags, vis,
                                          (const long long *)indptr, (long long)nnz, (const long long *)gaussian_ids,
                                          (const float4 *)g2d, v_comps, v_depths, scratch);
      };
      if (vis) launch(viewmat_partial_kernel<Form, false, CM>); else launch(viewmat_partial_kernel<Form, true, CM>);
    });
  viewmat_fold_kernel<<<C, kVg, 0, s>>>(scratch, B, v_viewmats);
}

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
  launch_viewmats(QuatScaleForm{means, quats, scales, opacities}, viewmats, Ks, N, C, width, height, eps2d, flags,
                  (const float4 *)splat, indptr, nnz, gaussian_ids, g2d, v_comps, v_depths, scratch, B, v_viewmats,
                  as_stream(stream));
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
  launch_viewmats(CovarForm{means, covars, nullptr}, viewmats, Ks, N, C, width, height, eps2d, flags, radii, indptr, nnz,
                  gaussian_ids, g2d, v_comps, v_depths, scratch, B, v_viewmats, as_stream(stream));
  return check_launch("project_covars_bwd_viewmats");
}
