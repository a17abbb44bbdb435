// Device code of the projection from covariances shared by functional.hip (the dense backward), packed.hip (the packed
// backwards) and viewmat_grad.hip (the camera-pose gradient): the reverse sweep of ONE visible (camera, Gaussian) pair
// behind forward_geom_covar (csrc/project_dev.h).  Every kernel that inlines it forms the same rounding sequence.
#pragma once
#include "project_dev.h"

namespace eg {

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
  // conic = B^-1  =>  G = -A V A with V = [[va, vb/2],[vb/2, vc]] (b is stored once): backward_geom's sweep
  const float hb = 0.5f * vb;
  const float av00 = f.a * va + f.b * hb, av01 = f.a * hb + f.b * vc;
  const float av10 = f.b * va + f.c * hb, av11 = f.b * hb + f.c * vc;
  float G00 = -(av00 * f.a + av01 * f.b);
  float G01 = -(av00 * f.b + av01 * f.c);
  float G11 = -(av10 * f.b + av11 * f.c);
  if (ct.has_comp) {
    // gsplat's 0.5 v / (comp + 1e-6); nothing where the determinant ratio is negative (comp is clamped to 0 there)
    const float det_conic = f.a * f.c - f.b * f.b;
    const float vs = (f.det0 / f.det1 >= 0.f) ? ct.v_comp * 0.5f / (f.comp + 1e-6f) : 0.f;
    const float omc = 1.f - f.comp * f.comp;
    G00 += vs * (omc * f.a - eps2d * det_conic);
    G01 += vs * (omc * f.b);
    G11 += vs * (omc * f.c - eps2d * det_conic);
  }
  float vcc[9];
  float vtx, vty, vtz;
  if constexpr (CM == kOrtho) {
    // cov2d = J cc J^T with the constant J = [[fx, 0, 0], [0, fy, 0]]: v_cc = J^T G J has the upper-left block only;
    // camera-space mean: through mean2d and the depth
    vcc[0] = f.J00 * f.J00 * G00;
    vcc[1] = vcc[3] = f.J00 * f.J11 * G01;
    vcc[4] = f.J11 * f.J11 * G11;
    vcc[2] = vcc[6] = vcc[5] = vcc[7] = vcc[8] = 0.f;
    vtx = cam.fx * vx;
    vty = cam.fy * vy;
    vtz = ct.v_depth;
  } else {
    // cov2d = J cc J^T (cc symmetric)  =>  v_J = 2 G Q with Q = J cc, v_cc = J^T G J
    const float vJ00 = 2.f * (G00 * q0[0] + G01 * q1[0]);
    const float vJ02 = 2.f * (G00 * q0[2] + G01 * q1[2]);
    const float vJ11 = 2.f * (G01 * q0[1] + G11 * q1[1]);
    const float vJ12 = 2.f * (G01 * q0[2] + G11 * q1[2]);
    const float g0 = G00 * f.J02 + G01 * f.J12, g1 = G01 * f.J02 + G11 * f.J12;  // G J[:, 2]
    vcc[0] = f.J00 * f.J00 * G00;
    vcc[1] = vcc[3] = f.J00 * f.J11 * G01;
    vcc[2] = vcc[6] = f.J00 * g0;
    vcc[4] = f.J11 * f.J11 * G11;
    vcc[5] = vcc[7] = f.J11 * g1;
    vcc[8] = f.J02 * g0 + f.J12 * g1;
    // camera-space mean: through mean2d, the depth and J (fov clamp freezes tx = +-lim z)
    const float rz3 = f.rz2 * f.rz;
    vtx = cam.fx * f.rz * vx;
    vty = cam.fy * f.rz * vy;
    vtz = -(cam.fx * f.x * vx + cam.fy * f.y * vy) * f.rz2 + ct.v_depth;
    vtz += -cam.fx * f.rz2 * vJ00 - cam.fy * f.rz2 * vJ11;
    if (f.in_x) { vtx += -cam.fx * f.rz2 * vJ02; vtz += 2.f * cam.fx * f.tx * rz3 * vJ02; }
    else        { vtz += cam.fx * f.tx * rz3 * vJ02; }
    if (f.in_y) { vty += -cam.fy * f.rz2 * vJ12; vtz += 2.f * cam.fy * f.ty * rz3 * vJ12; }
    else        { vtz += cam.fy * f.ty * rz3 * vJ12; }
  }
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

}  // namespace eg
