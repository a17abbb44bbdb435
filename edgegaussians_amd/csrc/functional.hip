// The three stages of gsplat's functional API that had no kernel (edgegaussians_amd/functional.py):
//
//   quat_scale_to_covar_preci   covar = R diag(s^2) R^T and / or preci = R diag(1 / s^2) R^T, full [N,3,3] or the upper
//                               triangle [N,6] = (00, 01, 02, 11, 12, 22), with the VJP.  One lane per Gaussian.
//   projection from covariances gsplat `fully_fused_projection(means, covars=[N,6], quats=None, scales=None)` for C
//                               cameras (packed=False) with the VJP.  Forward: grid (ceil(N / 256), C), one lane per
//                               pair, forward_geom_covar + radius_of (csrc/project_dev.h), zeros on a culled row.
//                               The `_flags` entry pair takes the camera model (EG_FLAG_ORTHO), a template parameter.
//                               Backward: one lane per Gaussian walks the cameras 0 .. C-1, recomputes the forward of the
//                               pairs with radii > 0, sums in registers and writes every row once (eg_packed_bwd's and
//                               eg_sh_bwd's scheme): no atomics, no zero-fill, the same bits every run.
//   isect_offset_encode         offsets[c, t] = number of entries of a caller's sorted isect ids below (c, t): one
//                               thread per entry compares its (camera, tile) with its predecessor's and fills the gap.
//
// The upper-triangle convention of every gradient here: an off-diagonal entry of a [N,6] tensor stands for BOTH
// symmetric entries of the matrix -- the gradient autograd gives through "build the matrix, select the upper triangle"
// (outputs) and through "place the six numbers into the symmetric matrix" (inputs).
#include "common.h"
#include "covar_dev.h"
#include "project_dev.h"

namespace eg {

constexpr int kFn = 256;  // threads per workgroup of every kernel here

struct QuatRot {
  float w, x, y, z, qinv, R[9];
};

// (w, x, y, z) -> rotation; normalised with rsqrtf of the squared norm, as forward_geom does
__device__ __forceinline__ QuatRot quat_rot(const float *__restrict__ q) {
#pragma clang fp contract(off)  // (the full and the upper-triangle forms give the same bits)
  QuatRot r;
  float w = q[0], x = q[1], y = q[2], z = q[3];
  r.qinv = rsqrtf(w * w + x * x + y * y + z * z);
  w *= r.qinv; x *= r.qinv; y *= r.qinv; z *= r.qinv;
  r.w = w; r.x = x; r.y = y; r.z = z;
  const float x2 = x * x, y2 = y * y, z2 = z * z, xy = x * y, xz = x * z, yz = y * z;
  const float wx = w * x, wy = w * y, wz = w * z;
  r.R[0] = 1.f - 2.f * (y2 + z2); r.R[1] = 2.f * (xy - wz);       r.R[2] = 2.f * (xz + wy);
  r.R[3] = 2.f * (xy + wz);       r.R[4] = 1.f - 2.f * (x2 + z2); r.R[5] = 2.f * (yz - wx);
  r.R[6] = 2.f * (xz - wy);       r.R[7] = 2.f * (yz + wx);       r.R[8] = 1.f - 2.f * (x2 + y2);
  return r;
}

// upper triangle of M M^T, M = R diag(d)
__device__ __forceinline__ void rdr(const float *R, const float *d, float (&o)[6]) {
#pragma clang fp contract(off)
  float M[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) M[3 * i + k] = R[3 * i + k] * d[k];
  constexpr int ui[6] = {0, 0, 0, 1, 1, 2}, uj[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
  for (int e = 0; e < 6; ++e)
    o[e] = M[3 * ui[e]] * M[3 * uj[e]] + M[3 * ui[e] + 1] * M[3 * uj[e] + 1] + M[3 * ui[e] + 2] * M[3 * uj[e] + 2];
}

__device__ __forceinline__ void store_sym(float *__restrict__ out, int g, const float (&u)[6], bool triu) {
  if (triu) {
#pragma unroll
    for (int e = 0; e < 6; ++e) out[6 * (size_t)g + e] = u[e];
  } else {
    float *o = out + 9 * (size_t)g;
    o[0] = u[0]; o[1] = u[1]; o[2] = u[2];
    o[3] = u[1]; o[4] = u[3]; o[5] = u[4];
    o[6] = u[2]; o[7] = u[4]; o[8] = u[5];
  }
}

__global__ void __launch_bounds__(kFn)
qs2cp_fwd_kernel(const float *__restrict__ quats, const float *__restrict__ scales, int N, int triu,
                 float *__restrict__ covars, float *__restrict__ precis) {
#pragma clang fp contract(off)
  const int g = blockIdx.x * kFn + threadIdx.x;
  if (g >= N) return;
  const QuatRot r = quat_rot(quats + 4 * (size_t)g);
  const float s[3] = {scales[3 * (size_t)g], scales[3 * (size_t)g + 1], scales[3 * (size_t)g + 2]};
  float u[6];
  if (covars) {
    rdr(r.R, s, u);
    store_sym(covars, g, u, triu);
  }
  if (precis) {
    const float si[3] = {1.f / s[0], 1.f / s[1], 1.f / s[2]};
    rdr(r.R, si, u);
    store_sym(precis, g, u, triu);
  }
}

// S = V + V^T of one cotangent: from the full [3,3] block, or from the six upper-triangle numbers
__device__ __forceinline__ void load_sym_cot(const float *__restrict__ v, int g, bool triu, float (&S)[9]) {
  if (triu) {
    const float *p = v + 6 * (size_t)g;
    S[0] = 2.f * p[0]; S[1] = p[1];       S[2] = p[2];
    S[3] = p[1];       S[4] = 2.f * p[3]; S[5] = p[4];
    S[6] = p[2];       S[7] = p[4];       S[8] = 2.f * p[5];
  } else {
    const float *p = v + 9 * (size_t)g;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) S[3 * i + j] = p[3 * i + j] + p[3 * j + i];
  }
}

// rotation cotangent -> raw quaternion cotangent (the tail of backward_geom)
__device__ __forceinline__ void rot_to_quat_vjp(const QuatRot &r, const float *vR, float *vq) {
#pragma clang fp contract(off)
  const float w = r.w, x = r.x, y = r.y, z = r.z;
  const float nw = 2.f * (x * (vR[7] - vR[5]) + y * (vR[2] - vR[6]) + z * (vR[3] - vR[1]));
  const float nx = 2.f * (-2.f * x * (vR[4] + vR[8]) + y * (vR[1] + vR[3]) + z * (vR[2] + vR[6]) + w * (vR[7] - vR[5]));
  const float ny = 2.f * (x * (vR[1] + vR[3]) - 2.f * y * (vR[0] + vR[8]) + z * (vR[5] + vR[7]) + w * (vR[2] - vR[6]));
  const float nz = 2.f * (x * (vR[2] + vR[6]) + y * (vR[5] + vR[7]) - 2.f * z * (vR[0] + vR[4]) + w * (vR[3] - vR[1]));
  const float d = nw * w + nx * x + ny * y + nz * z;
  vq[0] = (nw - d * w) * r.qinv;
  vq[1] = (nx - d * x) * r.qinv;
  vq[2] = (ny - d * y) * r.qinv;
  vq[3] = (nz - d * z) * r.qinv;
}

__global__ void __launch_bounds__(kFn)
qs2cp_bwd_kernel(const float *__restrict__ quats, const float *__restrict__ scales, int N, int triu,
                 const float *__restrict__ v_covars, const float *__restrict__ v_precis, float *__restrict__ v_quats,
                 float *__restrict__ v_scales) {
#pragma clang fp contract(off)
  const int g = blockIdx.x * kFn + threadIdx.x;
  if (g >= N) return;
  const QuatRot r = quat_rot(quats + 4 * (size_t)g);
  const float s[3] = {scales[3 * (size_t)g], scales[3 * (size_t)g + 1], scales[3 * (size_t)g + 2]};
  float vR[9], vs[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 9; ++k) vR[k] = 0.f;
  // out = M M^T, M = R diag(d)  =>  v_M = (V + V^T) M;  v_R = v_M diag(d), v_d[k] = sum_i R[i][k] v_M[i][k]
  float S[9];
  if (v_covars) {
    load_sym_cot(v_covars, g, triu, S);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float vM = (S[3 * i] * r.R[k] + S[3 * i + 1] * r.R[3 + k] + S[3 * i + 2] * r.R[6 + k]) * s[k];
        acc += r.R[3 * i + k] * vM;
        vR[3 * i + k] += vM * s[k];
      }
      vs[k] += acc;
    }
  }
  if (v_precis) {
    load_sym_cot(v_precis, g, triu, S);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float si = 1.f / s[k];
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float vM = (S[3 * i] * r.R[k] + S[3 * i + 1] * r.R[3 + k] + S[3 * i + 2] * r.R[6 + k]) * si;
        acc += r.R[3 * i + k] * vM;
        vR[3 * i + k] += vM * si;
      }
      vs[k] += -(acc * si) * si;  // d (1 / s) = -1 / s^2
    }
  }
  float vq[4];
  rot_to_quat_vjp(r, vR, vq);
#pragma unroll
  for (int k = 0; k < 4; ++k) v_quats[4 * (size_t)g + k] = vq[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) v_scales[3 * (size_t)g + k] = vs[k];
}

// ---------------------------------------------------------------------------------------------
// CM: the camera model (csrc/project_dev.h) of the two projection kernels: kPinhole behind eg_project_covars_{fwd,bwd}_cams,
// either behind eg_project_covars_{fwd,bwd}_cams_flags (kOrtho with EG_FLAG_ORTHO).
template <int CM>
__global__ void __launch_bounds__(kFn)
project_covars_fwd_kernel(const float *__restrict__ means, const float *__restrict__ covars,
                          const float *__restrict__ viewmats, const float *__restrict__ Ks, int N, int width,
                          int height, float near_plane, float far_plane, float eps2d, float radius_clip,
                          int *__restrict__ radii, float *__restrict__ means2d, float *__restrict__ depths,
                          float *__restrict__ conics, float *__restrict__ comps) {
  const int g = blockIdx.x * kFn + threadIdx.x;
  if (g >= N) return;
  const int c = blockIdx.y;
  const Cam cam = load_cam(viewmats + 16 * (size_t)c, Ks + 9 * (size_t)c);
  float m[3], cv[6], cc[6], q0[3], q1[3];
  load_mean_covar(means, covars, g, m, cv);
  Fwd f;
  int radius = 0;
  if (forward_geom_covar<CM>(cam, m, cv, width, height, near_plane, far_plane, eps2d, f, cc, q0, q1))
    radius = radius_of(f, width, height, radius_clip);
  const bool keep = radius > 0;
  const size_t p = (size_t)c * N + g;
  radii[p] = radius;
  means2d[2 * p] = keep ? f.u : 0.f;
  means2d[2 * p + 1] = keep ? f.v : 0.f;
  depths[p] = keep ? f.z : 0.f;
  conics[3 * p] = keep ? f.a : 0.f;
  conics[3 * p + 1] = keep ? f.b : 0.f;
  conics[3 * p + 2] = keep ? f.c : 0.f;
  if (comps) comps[p] = keep ? f.comp : 0.f;
}

template <int CM>
__global__ void __launch_bounds__(kFn)
project_covars_bwd_kernel(const float *__restrict__ means, const float *__restrict__ covars,
                          const float *__restrict__ viewmats, const float *__restrict__ Ks, int N, int C, int width,
                          int height, float eps2d, const int *__restrict__ radii, const float *__restrict__ v_means2d,
                          const float *__restrict__ v_depths, const float *__restrict__ v_conics,
                          const float *__restrict__ v_comps, float *__restrict__ v_means,
                          float *__restrict__ v_covars) {
#pragma clang fp contract(off)  // (the same bits whatever the compiler makes of the camera loop)
  const int g = blockIdx.x * kFn + threadIdx.x;
  if (g >= N) return;
  float m[3], cv[6];
  load_mean_covar(means, covars, g, m, cv);
  float am[3] = {0.f, 0.f, 0.f}, ac[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < C; ++c) {
    const size_t p = (size_t)c * N + g;
    if (radii[p] <= 0) continue;
    const Cam cam = load_cam(viewmats + 16 * (size_t)c, Ks + 9 * (size_t)c);
    Fwd f;
    float cc[6], q0[3], q1[3];
    // near / far already passed in the forward (the radius is positive), so pass open limits
    if (!forward_geom_covar<CM>(cam, m, cv, width, height, -3.0e38f, 3.0e38f, eps2d, f, cc, q0, q1)) continue;
    CovarCot ct;
    ct.vx = v_means2d[2 * p]; ct.vy = v_means2d[2 * p + 1];
    ct.va = v_conics[3 * p]; ct.vb = v_conics[3 * p + 1]; ct.vc = v_conics[3 * p + 2];
    ct.v_depth = v_depths ? v_depths[p] : 0.f;
    ct.has_comp = v_comps != nullptr;
    ct.v_comp = v_comps ? v_comps[p] : 0.f;
    float gm[3], gc[6];
    covar_pair_vjp<false, CM>(cam, m, cv, f, q0, q1, eps2d, ct, gm, gc);  // (csrc/covar_dev.h)
#pragma unroll
    for (int k = 0; k < 3; ++k) am[k] += gm[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) ac[k] += gc[k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) v_means[3 * (size_t)g + k] = am[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) v_covars[6 * (size_t)g + k] = ac[k];
}

// ---------------------------------------------------------------------------------------------
// (camera, tile) of an isect id as one index c * T + t, clamped into [0, CT - 1] (ids outside the grid write nowhere
// outside `offsets`)
__device__ __forceinline__ long long isect_cell(long long id, int tile_bits, int T, long long CT) {
  const unsigned long long key = (unsigned long long)id >> 32;
  const long long cam = (long long)(key >> tile_bits), tile = (long long)(key & ((1ull << tile_bits) - 1ull));
  const long long cell = cam * T + tile;
  return cell < 0 ? 0 : (cell >= CT ? CT - 1 : cell);
}

__global__ void __launch_bounds__(kFn)
isect_offset_encode_kernel(const long long *__restrict__ isect_ids, long long M, int tile_bits, int T, long long CT,
                           int *__restrict__ offsets) {
  const long long i = blockIdx.x * (long long)kFn + threadIdx.x;
  if (M == 0) {  // (no entries: every cell starts at 0)
    if (i < CT) offsets[i] = 0;
    return;
  }
  if (i >= M) return;
  const long long cur = isect_cell(isect_ids[i], tile_bits, T, CT);
  const long long prev = i == 0 ? -1 : isect_cell(isect_ids[i - 1], tile_bits, T, CT);
  for (long long j = prev + 1; j <= cur; ++j) offsets[j] = (int)i;  // (empty when the entry continues a run)
  if (i == M - 1)
    for (long long j = cur + 1; j < CT; ++j) offsets[j] = (int)M;
}

}  // namespace eg

using namespace eg;

extern "C" int eg_quat_scale_to_covar_preci_fwd(const float *quats, const float *scales, int32_t N, int32_t triu,
                                                float *covars, float *precis, eg_stream_t stream) {
  EG_REQUIRE(N >= 0, "bad sizes");
  if (N == 0) return EG_OK;
  EG_REQUIRE(quats && scales, "null pointer");
  if (!covars && !precis) return EG_OK;
  qs2cp_fwd_kernel<<<cdiv(N, kFn), kFn, 0, as_stream(stream)>>>(quats, scales, N, triu, covars, precis);
  return check_launch("quat_scale_to_covar_preci_fwd");
}

extern "C" int eg_quat_scale_to_covar_preci_bwd(const float *quats, const float *scales, int32_t N, int32_t triu,
                                                const float *v_covars, const float *v_precis, float *v_quats,
                                                float *v_scales, eg_stream_t stream) {
  EG_REQUIRE(N >= 0, "bad sizes");
  if (N == 0) return EG_OK;
  EG_REQUIRE(quats && scales && v_quats && v_scales, "null pointer");
  qs2cp_bwd_kernel<<<cdiv(N, kFn), kFn, 0, as_stream(stream)>>>(quats, scales, N, triu, v_covars, v_precis, v_quats,
                                                               v_scales);
  return check_launch("quat_scale_to_covar_preci_bwd");
}

// the two launches behind both entry pairs; the camera model comes from the flags (0 = pinhole)
static void launch_project_covars_fwd(const float *means, const float *covars, const float *viewmats, const float *Ks,
                                      int32_t N, int32_t C, int32_t width, int32_t height, float near_plane,
                                      float far_plane, float eps2d, float radius_clip, int32_t *radii, float *means2d,
                                      float *depths, float *conics, float *compensations, uint32_t flags,
                                      eg_stream_t stream) {
  with_cam_model(flags, [&](auto cm) {
    project_covars_fwd_kernel<decltype(cm)::value><<<dim3(cdiv(N, kFn), C), kFn, 0, as_stream(stream)>>>(
        means, covars, viewmats, Ks, N, width, height, near_plane, far_plane, eps2d, radius_clip, radii, means2d, depths,
        conics, compensations);
  });
}

static void launch_project_covars_bwd(const float *means, const float *covars, const float *viewmats, const float *Ks,
                                      int32_t N, int32_t C, int32_t width, int32_t height, float eps2d,
                                      const int32_t *radii, const float *v_means2d, const float *v_depths,
                                      const float *v_conics, const float *v_compensations, float *v_means,
                                      float *v_covars, uint32_t flags, eg_stream_t stream) {
  with_cam_model(flags, [&](auto cm) {
    project_covars_bwd_kernel<decltype(cm)::value><<<cdiv(N, kFn), kFn, 0, as_stream(stream)>>>(
        means, covars, viewmats, Ks, N, C, width, height, eps2d, radii, v_means2d, v_depths, v_conics, v_compensations,
        v_means, v_covars);
  });
}

extern "C" int eg_project_covars_fwd_cams(const float *means, const float *covars, const float *viewmats,
                                          const float *Ks, int32_t N, int32_t C, int32_t width, int32_t height,
                                          float near_plane, float far_plane, float eps2d, float radius_clip,
                                          int32_t *radii, float *means2d, float *depths, float *conics,
                                          float *compensations, eg_stream_t stream) {
  EG_REQUIRE(N >= 0 && C >= 1 && C <= 65535 && width > 0 && height > 0, "bad sizes");
  if (N == 0) return EG_OK;
  EG_REQUIRE(means && covars && viewmats && Ks && radii && means2d && depths && conics, "null pointer");
  launch_project_covars_fwd(means, covars, viewmats, Ks, N, C, width, height, near_plane, far_plane, eps2d, radius_clip,
                            radii, means2d, depths, conics, compensations, 0, stream);
  return check_launch("project_covars_fwd_cams");
}

// the same projection with a camera model: flags = 0 (pinhole) or EG_FLAG_ORTHO
extern "C" int eg_project_covars_fwd_cams_flags(const float *means, const float *covars, const float *viewmats,
                                                const float *Ks, int32_t N, int32_t C, int32_t width, int32_t height,
                                                float near_plane, float far_plane, float eps2d, float radius_clip,
                                                int32_t *radii, float *means2d, float *depths, float *conics,
                                                float *compensations, uint32_t flags, eg_stream_t stream) {
  EG_REQUIRE(N >= 0 && C >= 1 && C <= 65535 && width > 0 && height > 0, "bad sizes");
  EG_REQUIRE(!(flags & ~EG_FLAG_ORTHO), "flags: EG_FLAG_ORTHO or 0");
  if (N == 0) return EG_OK;
  EG_REQUIRE(means && covars && viewmats && Ks && radii && means2d && depths && conics, "null pointer");
  launch_project_covars_fwd(means, covars, viewmats, Ks, N, C, width, height, near_plane, far_plane, eps2d, radius_clip,
                            radii, means2d, depths, conics, compensations, flags, stream);
  return check_launch("project_covars_fwd_cams_flags");
}

extern "C" int eg_project_covars_bwd_cams(const float *means, const float *covars, const float *viewmats,
                                          const float *Ks, int32_t N, int32_t C, int32_t width, int32_t height,
                                          float eps2d, const int32_t *radii, const float *v_means2d,
                                          const float *v_depths, const float *v_conics, const float *v_compensations,
                                          float *v_means, float *v_covars, eg_stream_t stream) {
  EG_REQUIRE(N >= 0 && C >= 1 && width > 0 && height > 0, "bad sizes");
  if (N == 0) return EG_OK;
  EG_REQUIRE(means && covars && viewmats && Ks && radii && v_means2d && v_conics && v_means && v_covars, "null pointer");
  launch_project_covars_bwd(means, covars, viewmats, Ks, N, C, width, height, eps2d, radii, v_means2d, v_depths, v_conics,
                            v_compensations, v_means, v_covars, 0, stream);
  return check_launch("project_covars_bwd_cams");
}

extern "C" int eg_project_covars_bwd_cams_flags(const float *means, const float *covars, const float *viewmats,
                                                const float *Ks, int32_t N, int32_t C, int32_t width, int32_t height,
                                                float eps2d, const int32_t *radii, const float *v_means2d,
                                                const float *v_depths, const float *v_conics,
                                                const float *v_compensations, float *v_means, float *v_covars,
                                                uint32_t flags, eg_stream_t stream) {
  EG_REQUIRE(N >= 0 && C >= 1 && width > 0 && height > 0, "bad sizes");
  EG_REQUIRE(!(flags & ~EG_FLAG_ORTHO), "flags: EG_FLAG_ORTHO or 0");
  if (N == 0) return EG_OK;
  EG_REQUIRE(means && covars && viewmats && Ks && radii && v_means2d && v_conics && v_means && v_covars, "null pointer");
  launch_project_covars_bwd(means, covars, viewmats, Ks, N, C, width, height, eps2d, radii, v_means2d, v_depths, v_conics,
                            v_compensations, v_means, v_covars, flags, stream);
  return check_launch("project_covars_bwd_cams_flags");
}

extern "C" int eg_isect_offset_encode(const int64_t *isect_ids, int64_t M, int32_t C, int32_t tile_width,
                                      int32_t tile_height, int32_t *offsets, eg_stream_t stream) {
  EG_REQUIRE(M >= 0 && M < (1ll << 31) && C >= 1 && tile_width > 0 && tile_height > 0, "bad sizes");
  const int64_t T64 = (int64_t)tile_width * tile_height;
  EG_REQUIRE(T64 < (1ll << 30) && T64 * C < (1ll << 31), "bad sizes");
  EG_REQUIRE(offsets && (M == 0 || isect_ids), "null pointer");
  const int T = (int)T64;
  const long long CT = (long long)T * C;
  isect_offset_encode_kernel<<<cdiv(M > 0 ? M : CT, kFn), kFn, 0, as_stream(stream)>>>(
      (const long long *)isect_ids, (long long)M, tile_bits(T), T, CT, offsets);
  return check_launch("isect_offset_encode");
}
