// Device code of the projection from covariances shared by functional.hip (the dense backward), packed.hip (the packed
// backwards) and viewmat_grad.hip (the camera-pose gradient): the reverse sweep of ONE visible (camera, Gaussian) pair
// behind forward_geom_covar (csrc/project_dev.h), built from the steps it shares with backward_geom.  Every kernel that
// inlines it forms the same rounding sequence.  CovarForm (bottom) is what the kernels written once for both shape forms
// (packed.hip, viewmat_grad.hip) know of this one.
#pragma once
#include "project_dev.h"

namespace eg {

// world mean m[3] and covariance cv[6] (upper triangle) of Gaussian g
__device__ __forceinline__ void load_mean_covar(const float *__restrict__ means, const float *__restrict__ covars, int g,
                                                float (&m)[3], float (&cv)[6]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) m[k] = means[3 * (size_t)g + k];
#pragma unroll
  for (int k = 0; k < 6; ++k) cv[k] = covars[6 * (size_t)g + k];
}

// the cotangents of one pair's projection outputs (has_comp: the compensation has a cotangent at all)
struct CovarCot {
  float vx, vy;      // v_means2d
  float va, vb, vc;  // v_conics (b is stored once)
  float v_depth;
  float v_comp;
  bool has_comp;
};

// the [nnz, 8] / [C, N, 8] record of the compositing backwards (words 0-1 v_means2d, 4-6 v_conics) + v_comps + v_depths
__device__ __forceinline__ CovarCot load_covar_cot(const float4 *__restrict__ g2d, const float *__restrict__ v_comps,
                                                   const float *__restrict__ v_depths, long long p, bool has_comp) {
  const float4 ga = g2d[2 * p], gb = g2d[2 * p + 1];
  CovarCot ct;
  ct.vx = ga.x; ct.vy = ga.y;
  ct.va = gb.x; ct.vb = gb.y; ct.vc = gb.z;
  ct.v_depth = v_depths ? v_depths[p] : 0.f;
  ct.has_comp = has_comp;
  ct.v_comp = has_comp ? v_comps[p] : 0.f;
  return ct;
}

// The reverse sweep of one pair: `f`, q0, q1 from forward_geom_covar<CM>(cam, m, cv, ...).  v_mean[3] and v_cov[6] are
// the pair's share of the gradients of the world mean and of the six upper-triangle numbers (an off-diagonal stands for
// both symmetric entries); the caller sums them over the cameras.
// CAM (csrc/viewmat_grad.hip): the same sweep stops at the camera-space cotangents and leaves the CAMERA's share in
// v_cam[12] -- rows of [v_R | v_tr]: from cc = Rv S Rv^T and t = Rv m + tr, v_R = v_t m^T + (v_cc + v_cc^T) Rv S and
// v_tr = v_t -- v_mean and v_cov are not touched.
template <bool CAM, int CM>
__device__ __forceinline__ void covar_pair_vjp(const Cam &cam, const float *m, const float *cv, const Fwd &f,
                                               const float (&q0)[3], const float (&q1)[3], float eps2d,
                                               const CovarCot &ct, float *v_mean, float *v_cov,
                                               float *v_cam = nullptr) {
#pragma clang fp contract(off)  // (the same bits whatever the compiler makes of the caller's camera loop)
  const float vx = ct.vx, vy = ct.vy;
  const float va = ct.va, vb = ct.vb, vc = ct.vc;
  float G00, G01, G11;
  conic_vjp(f, va, vb, vc, G00, G01, G11);
  if (ct.has_comp) comp_vjp<true>(f, eps2d, ct.v_comp, G00, G01, G11);
  // cov2d = J cc J^T (cc symmetric)  =>  v_cc = J^T G J and -- pinhole -- v_J = 2 G Q with Q = J cc.  Ortho: the
  // constant J = [[fx, 0, 0], [0, fy, 0]] has no cotangent and v_cc the upper-left block only.
  float vcc[9];
  float vJ00 = 0.f, vJ02 = 0.f, vJ11 = 0.f, vJ12 = 0.f;
  vcc[0] = f.J00 * f.J00 * G00;
  vcc[1] = vcc[3] = f.J00 * f.J11 * G01;
  vcc[4] = f.J11 * f.J11 * G11;
  if constexpr (CM == kOrtho) {
    vcc[2] = vcc[6] = vcc[5] = vcc[7] = vcc[8] = 0.f;
  } else {
    vJ00 = 2.f * (G00 * q0[0] + G01 * q1[0]);
    vJ02 = 2.f * (G00 * q0[2] + G01 * q1[2]);
    vJ11 = 2.f * (G01 * q0[1] + G11 * q1[1]);
    vJ12 = 2.f * (G01 * q0[2] + G11 * q1[2]);
    const float g0 = G00 * f.J02 + G01 * f.J12, g1 = G01 * f.J02 + G11 * f.J12;  // G J[:, 2]
    vcc[2] = vcc[6] = f.J00 * g0;
    vcc[5] = vcc[7] = f.J11 * g1;
    vcc[8] = f.J02 * g0 + f.J12 * g1;
  }
  float vtx, vty, vtz;
  camera_mean_vjp<CM>(cam, f, vx, vy, ct.v_depth, vJ00, vJ02, vJ11, vJ12, vtx, vty, vtz);
  if constexpr (CAM) {
    // A = Rv S (forward_geom_covar's first product); v_cc is symmetric as built, so v_cc + v_cc^T = 2 v_cc
    const float S[9] = {cv[0], cv[1], cv[2], cv[1], cv[3], cv[4], cv[2], cv[4], cv[5]};
    float A[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k)
        A[3 * i + k] = cam.R[3 * i] * S[k] + cam.R[3 * i + 1] * S[3 + k] + cam.R[3 * i + 2] * S[6 + k];
    const float vt[3] = {vtx, vty, vtz};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        v_cam[4 * i + j] = vt[i] * m[j] + 2.f * (vcc[3 * i] * A[j] + vcc[3 * i + 1] * A[3 + j] + vcc[3 * i + 2] * A[6 + j]);
      v_cam[4 * i + 3] = vt[i];
    }
    return;
  }
  v_mean[0] = cam.R[0] * vtx + cam.R[3] * vty + cam.R[6] * vtz;
  v_mean[1] = cam.R[1] * vtx + cam.R[4] * vty + cam.R[7] * vtz;
  v_mean[2] = cam.R[2] * vtx + cam.R[5] * vty + cam.R[8] * vtz;
  // cc = Rv S Rv^T  =>  v_S = Rv^T v_cc Rv; an off-diagonal of the six stands for both symmetric entries
  float B[9];  // v_cc Rv
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      B[3 * i + k] = vcc[3 * i] * cam.R[k] + vcc[3 * i + 1] * cam.R[3 + k] + vcc[3 * i + 2] * cam.R[6 + k];
  constexpr int ui[6] = {0, 0, 0, 1, 1, 2}, uj[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
  for (int e = 0; e < 6; ++e) {
    const float vS = cam.R[ui[e]] * B[uj[e]] + cam.R[3 + ui[e]] * B[3 + uj[e]] + cam.R[6 + ui[e]] * B[6 + uj[e]];
    v_cov[e] = (ui[e] == uj[e]) ? vS : 2.f * vS;
  }
}

// ---------------------------------------------------------------------------------------------
// The covariance form of a Gaussian's shape (covars [N, 6]), member for member QuatScaleForm's counterpart
// (csrc/project_dev.h).  The host fills the three pointers (opacities: the write pass only); m, cv, q0, q1 are the
// kernel's (forward() fills them, pair_vjp reads them).
struct CovarForm {
  const float *means, *covars, *opacities;
  float m[3], cv[6], q0[3], q1[3];

  using Visible = int;  // the dense layout's radii [C, N]
  static __device__ __forceinline__ bool visible(const int *radii, long long q) { return radii[q] > 0; }

  template <int CM>
  __device__ __forceinline__ bool forward(const Cam &cam, int g, int width, int height, float near_plane,
                                          float far_plane, float eps2d, uint32_t, Fwd &f) {
    load_mean_covar(means, covars, g, m, cv);
    float cc[6];
    return forward_geom_covar<CM>(cam, m, cv, width, height, near_plane, far_plane, eps2d, f, cc, q0, q1);
  }
  // (forward_geom_covar does not fill f.o: the record's opacity comes straight from opacities[g])
  __device__ __forceinline__ float opacity(const Fwd &, int g) const { return opacities[g]; }

  // one row of v_means [*, 3], v_covars [*, 6]
  struct Out {
    float *v_means, *v_covars;
  };
  struct Grad {
    float mean[3], cov[6];
    __device__ __forceinline__ void zero() {
#pragma unroll
      for (int k = 0; k < 3; ++k) mean[k] = 0.f;
#pragma unroll
      for (int k = 0; k < 6; ++k) cov[k] = 0.f;
    }
    __device__ __forceinline__ void operator+=(const Grad &o) {
#pragma clang fp contract(off)  // (the same bits whatever the compiler makes of the caller's camera loop)
#pragma unroll
      for (int k = 0; k < 3; ++k) mean[k] += o.mean[k];
#pragma unroll
      for (int k = 0; k < 6; ++k) cov[k] += o.cov[k];
    }
    __device__ __forceinline__ void store(const Out &out, long long row) const {
#pragma unroll
      for (int k = 0; k < 3; ++k) out.v_means[3 * row + k] = mean[k];
#pragma unroll
      for (int k = 0; k < 6; ++k) out.v_covars[6 * row + k] = cov[k];
    }
  };

  // pair p = (cam, g) of a visible list: its share of the row's gradient, or (CAM) the camera's share in v_cam[12].
  // Near / far passed in the forward, so the recomputation runs with open limits; should its det cull strike, `gr` and
  // `v_cam` stay as the caller zeroed them.  The compensation has a cotangent under EG_FLAG_ANTIALIASED only.
  template <bool CAM, int CM>
  __device__ __forceinline__ void pair_vjp(const Cam &cam, int g, long long p, int width, int height, float eps2d,
                                           uint32_t flags, const float4 *__restrict__ g2d,
                                           const float *__restrict__ v_comps, const float *__restrict__ v_depths,
                                           Grad &gr, float *v_cam = nullptr) {
    Fwd f;
    if (!forward<CM>(cam, g, width, height, -3.0e38f, 3.0e38f, eps2d, flags, f)) return;
    const CovarCot ct = load_covar_cot(g2d, v_comps, v_depths, p, flags & EG_FLAG_ANTIALIASED);
    covar_pair_vjp<CAM, CM>(cam, m, cv, f, q0, q1, eps2d, ct, gr.mean, gr.cov, v_cam);
  }
};

}  // namespace eg
