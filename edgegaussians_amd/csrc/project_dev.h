// Device code of the projection (G1 / G9) shared by every kernel that projects: camera, the forward geometry of one
// Gaussian from quats + scales (forward_geom) or from a covariance (forward_geom_covar), the reverse sweep
// (backward_geom; the covariance's is csrc/covar_dev.h), Adam.  The halves the two forms have in common -- camera-space
// mean and near / far cull, the camera model's J and mean2d, cov2d -> conic, and their reverse steps -- are helpers
// written once; each carries its own `fp contract(off)` (the pragma is lexical, it does not follow an inlined call), so
// every kernel that inlines them forms the SAME rounding sequence -- see the comment inside forward_geom.
// QuatScaleForm (bottom) is what the kernels written once for both forms (packed.hip, viewmat_grad.hip) know of this one.
#pragma once
#include <math.h>

#include <type_traits>

#include "common.h"

namespace eg {

struct Cam {
  float R[9], t[3], fx, fy, cx, cy;
};

// Camera model, a COMPILE-TIME parameter of forward_geom / forward_geom_covar / backward_geom (default: pinhole, the only
// model the training kernels instantiate).  kOrtho (EG_FLAG_ORTHO on the operator path, gsplat camera_model="ortho"):
// mean2d = (fx x + cx, fy y + cy), J = [[fx, 0, 0], [0, fy, 0]] -- no division by z, no fov clamp, cov2d independent of
// the mean; culls, depth and everything behind cov2d are the pinhole's.
enum CamModel : int { kPinhole = 0, kOrtho = 1 };

// host: the camera model of a launch as a compile-time value -- fn(cm) with decltype(cm)::value = kOrtho under
// EG_FLAG_ORTHO, kPinhole otherwise
template <class F>
inline void with_cam_model(uint32_t flags, F &&fn) {
  if (flags & EG_FLAG_ORTHO) fn(std::integral_constant<int, kOrtho>{}); else fn(std::integral_constant<int, kPinhole>{});
}

__device__ __forceinline__ Cam load_cam(const float *__restrict__ vm, const float *__restrict__ K) {
  Cam c;
  c.R[0] = vm[0]; c.R[1] = vm[1]; c.R[2] = vm[2];  c.t[0] = vm[3];
  c.R[3] = vm[4]; c.R[4] = vm[5]; c.R[5] = vm[6];  c.t[1] = vm[7];
  c.R[6] = vm[8]; c.R[7] = vm[9]; c.R[8] = vm[10]; c.t[2] = vm[11];
  c.fx = K[0]; c.cx = K[2]; c.fy = K[4]; c.cy = K[5];
  return c;
}

// Everything the forward computes for one visible Gaussian; the backward re-derives it instead of
// reading it back from memory (recompute is ~100 flops, a reload would be ~100 B).
struct Fwd {
  float x, y, z;            // camera-space mean
  float qw, qx, qy, qz, qinv;  // normalised quaternion and 1/|q|
  float s[3];               // scales (after exp)
  float o;                  // opacity (after sigmoid)
  float Rq[9];              // rotation of the Gaussian
  float W[9];               // Rv * Rq * diag(s)
  float rz, rz2, tx, ty;    // 1/z, 1/z^2, clamped x, y
  bool in_x, in_y;          // fov clamp inactive
  float J00, J02, J11, J12;
  float p0[3], p1[3];
  float c00, c01, c11, b00, b11, det0, det1;
  float a, b, c, comp;      // conic, compensation
  float u, v;               // mean2d
};

// the raw parameters of one Gaussian (as stored: log-scales / logit-opacity when the flags say so)
struct Raw {
  float m[3], q[4], s[3], o;
};
__device__ __forceinline__ Raw load_raw(const float *__restrict__ means, const float *__restrict__ quats,
                                        const float *__restrict__ scales, const float *__restrict__ opacities, int g) {
  Raw r;
#pragma unroll
  for (int k = 0; k < 3; ++k) { r.m[k] = means[3 * g + k]; r.s[k] = scales[3 * g + k]; }
#pragma unroll
  for (int k = 0; k < 4; ++k) r.q[k] = quats[4 * g + k];
  r.o = opacities[g];
  return r;
}

// The three steps of the forward that both shape forms share.  (No FMA contraction: see forward_geom.)
// camera-space mean of the world mean m[3]; false = outside [near_plane, far_plane]
__device__ __forceinline__ bool camera_mean(const Cam &cam, const float *m, float near_plane, float far_plane, Fwd &f) {
#pragma clang fp contract(off)
  const float mx = m[0], my = m[1], mz = m[2];
  f.x = cam.R[0] * mx + cam.R[1] * my + cam.R[2] * mz + cam.t[0];
  f.y = cam.R[3] * mx + cam.R[4] * my + cam.R[5] * mz + cam.t[1];
  f.z = cam.R[6] * mx + cam.R[7] * my + cam.R[8] * mz + cam.t[2];
  return !(f.z < near_plane || f.z > far_plane);
}

// the camera model at the camera-space mean: 1/z, the fov clamp, the Jacobian J and mean2d
template <int CM>
__device__ __forceinline__ void camera_jacobian(const Cam &cam, int width, int height, Fwd &f) {
#pragma clang fp contract(off)
  if constexpr (CM == kOrtho) {
    // J = [[fx, 0, 0], [0, fy, 0]]; the pinhole-only fields read as "no clamp"
    f.rz = 0.f; f.rz2 = 0.f;
    f.in_x = true; f.in_y = true;
    f.tx = f.x; f.ty = f.y;
    f.J00 = cam.fx; f.J11 = cam.fy;
    f.J02 = 0.f; f.J12 = 0.f;
    f.u = cam.fx * f.x + cam.cx;
    f.v = cam.fy * f.y + cam.cy;
  } else {
    const float lim_x = kFovClamp * (0.5f * (float)width / cam.fx);
    const float lim_y = kFovClamp * (0.5f * (float)height / cam.fy);
    f.rz = 1.f / f.z;
    f.rz2 = f.rz * f.rz;
    const float xr = f.x * f.rz, yr = f.y * f.rz;
    f.in_x = (xr <= lim_x) && (xr >= -lim_x);
    f.in_y = (yr <= lim_y) && (yr >= -lim_y);
    f.tx = f.z * fminf(lim_x, fmaxf(-lim_x, xr));
    f.ty = f.z * fminf(lim_y, fmaxf(-lim_y, yr));
    f.J00 = cam.fx * f.rz;
    f.J11 = cam.fy * f.rz;
    f.J02 = -cam.fx * f.tx * f.rz2;
    f.J12 = -cam.fy * f.ty * f.rz2;
    f.u = cam.fx * f.x * f.rz + cam.cx;
    f.v = cam.fy * f.y * f.rz + cam.cy;
  }
}

// cov2d (c00, c01, c11) -> determinants, blurred diagonal, compensation, conic; false = the det cull
__device__ __forceinline__ bool conic_of_cov2d(float eps2d, Fwd &f) {
#pragma clang fp contract(off)
  f.det0 = f.c00 * f.c11 - f.c01 * f.c01;
  f.b00 = f.c00 + eps2d;
  f.b11 = f.c11 + eps2d;
  f.det1 = f.b00 * f.b11 - f.c01 * f.c01;
  if (f.det1 <= 0.f) return false;
  f.comp = sqrtf(fmaxf(0.f, f.det0 / f.det1));
  const float inv = 1.f / f.det1;
  f.a = f.b11 * inv;
  f.b = -f.c01 * inv;
  f.c = f.b00 * inv;
  return true;
}

template <int CM = kPinhole>
__device__ __forceinline__ bool forward_geom(const Cam &cam, const Raw &raw, int width, int height,
                                             float near_plane, float far_plane, float eps2d, uint32_t flags,
                                             Fwd &f) {
  // No FMA contraction in here (nor in the tile tests of common.h): this function is inlined into four kernels
  // (project_fwd, project_emit, the projection backward's recomputation, the tail-fused next-view projection), and
  // the compiler's contraction choices differ from one inlining context to the next -- the packed records of the
  // operator path and of the training step then differ in the last bit, and with them a float-borderline tile hit
  // or alpha threshold here and there (1600 x 1200, 200 k Gaussians: one Gaussian's gradient off by 4e-4 of the
  // maximum between the two paths).  Separate multiplies and adds are also what the C oracle (gcc, x86-64) does.
#pragma clang fp contract(off)
  if (!camera_mean(cam, raw.m, near_plane, far_plane, f)) return false;

  float w = raw.q[0], x = raw.q[1], y = raw.q[2], z = raw.q[3];
  f.qinv = rsqrtf(w * w + x * x + y * y + z * z);
  w *= f.qinv; x *= f.qinv; y *= f.qinv; z *= f.qinv;
  f.qw = w; f.qx = x; f.qy = y; f.qz = z;
  const float x2 = x * x, y2 = y * y, z2 = z * z, xy = x * y, xz = x * z, yz = y * z;
  const float wx = w * x, wy = w * y, wz = w * z;
  f.Rq[0] = 1.f - 2.f * (y2 + z2); f.Rq[1] = 2.f * (xy - wz);       f.Rq[2] = 2.f * (xz + wy);
  f.Rq[3] = 2.f * (xy + wz);       f.Rq[4] = 1.f - 2.f * (x2 + z2); f.Rq[5] = 2.f * (yz - wx);
  f.Rq[6] = 2.f * (xz - wy);       f.Rq[7] = 2.f * (yz + wx);       f.Rq[8] = 1.f - 2.f * (x2 + y2);

#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float sv = raw.s[k];
    f.s[k] = (flags & EG_FLAG_LOG_SCALES) ? expf(sv) : sv;
  }
  const float ov = raw.o;
  f.o = (flags & EG_FLAG_LOGIT_OPACITIES) ? 1.f / (1.f + expf(-ov)) : ov;

  // W = Rv * (Rq * diag(s))
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      f.W[3 * i + k] =
          (cam.R[3 * i] * f.Rq[k] + cam.R[3 * i + 1] * f.Rq[3 + k] + cam.R[3 * i + 2] * f.Rq[6 + k]) * f.s[k];

  // P = J W (ortho: J = [[fx, 0, 0], [0, fy, 0]] takes the first two rows of W)
  camera_jacobian<CM>(cam, width, height, f);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if constexpr (CM == kOrtho) {
      f.p0[k] = f.J00 * f.W[k];
      f.p1[k] = f.J11 * f.W[3 + k];
    } else {
      f.p0[k] = f.J00 * f.W[k] + f.J02 * f.W[6 + k];
      f.p1[k] = f.J11 * f.W[3 + k] + f.J12 * f.W[6 + k];
    }
  }
  f.c00 = f.p0[0] * f.p0[0] + f.p0[1] * f.p0[1] + f.p0[2] * f.p0[2];
  f.c01 = f.p0[0] * f.p1[0] + f.p0[1] * f.p1[1] + f.p0[2] * f.p1[2];
  f.c11 = f.p1[0] * f.p1[0] + f.p1[1] * f.p1[1] + f.p1[2] * f.p1[2];
  return conic_of_cov2d(eps2d, f);
}

template <int CM = kPinhole>
__device__ __forceinline__ bool forward_geom(const Cam &cam, const float *__restrict__ means,
                                             const float *__restrict__ quats, const float *__restrict__ scales,
                                             const float *__restrict__ opacities, int g, int width, int height,
                                             float near_plane, float far_plane, float eps2d, uint32_t flags,
                                             Fwd &f) {
  return forward_geom<CM>(cam, load_raw(means, quats, scales, opacities, g), width, height, near_plane, far_plane, eps2d,
                          flags, f);
}

// Projection from a covariance (gsplat `fully_fused_projection(covars=[N,6])`, csrc/functional.hip): the world
// covariance arrives as its upper triangle cv = (00, 01, 02, 11, 12, 22) instead of quats + scales.  Fills the fields
// of `f` that radius_of and the reverse sweep of functional.hip read (camera-space mean, clamp, J, cov2d, conic,
// compensation, mean2d; the quaternion / scale / W / p0 / p1 fields stay untouched), the camera-space covariance
// cc (same six entries) and Q = J cc (rows q0, q1).  Same culls, clamp and rounding discipline as forward_geom.
template <int CM = kPinhole>
__device__ __forceinline__ bool forward_geom_covar(const Cam &cam, const float *__restrict__ m,
                                                   const float *__restrict__ cv, int width, int height,
                                                   float near_plane, float far_plane, float eps2d, Fwd &f,
                                                   float (&cc)[6], float (&q0)[3], float (&q1)[3]) {
#pragma clang fp contract(off)  // (one rounding sequence in every kernel: see forward_geom)
  if (!camera_mean(cam, m, near_plane, far_plane, f)) return false;

  // cc = Rv S Rv^T, S symmetric: A = Rv S, then the upper triangle of A Rv^T
  const float S[9] = {cv[0], cv[1], cv[2], cv[1], cv[3], cv[4], cv[2], cv[4], cv[5]};
  float A[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      A[3 * i + k] = cam.R[3 * i] * S[k] + cam.R[3 * i + 1] * S[3 + k] + cam.R[3 * i + 2] * S[6 + k];
  constexpr int ui[6] = {0, 0, 0, 1, 1, 2}, uj[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
  for (int e = 0; e < 6; ++e)
    cc[e] = A[3 * ui[e]] * cam.R[3 * uj[e]] + A[3 * ui[e] + 1] * cam.R[3 * uj[e] + 1] + A[3 * ui[e] + 2] * cam.R[3 * uj[e] + 2];

  // Q = J cc, cov2d = Q J^T (ortho: J = [[fx, 0, 0], [0, fy, 0]] scales the first two rows of cc, cov2d is the
  // upper-left block of Q J^T)
  camera_jacobian<CM>(cam, width, height, f);
  if constexpr (CM == kOrtho) {
    q0[0] = f.J00 * cc[0]; q0[1] = f.J00 * cc[1]; q0[2] = f.J00 * cc[2];
    q1[0] = f.J11 * cc[1]; q1[1] = f.J11 * cc[3]; q1[2] = f.J11 * cc[4];
    f.c00 = q0[0] * f.J00;
    f.c01 = q0[1] * f.J11;
    f.c11 = q1[1] * f.J11;
  } else {
    q0[0] = f.J00 * cc[0] + f.J02 * cc[2];
    q0[1] = f.J00 * cc[1] + f.J02 * cc[4];
    q0[2] = f.J00 * cc[2] + f.J02 * cc[5];
    q1[0] = f.J11 * cc[1] + f.J12 * cc[2];
    q1[1] = f.J11 * cc[3] + f.J12 * cc[4];
    q1[2] = f.J11 * cc[4] + f.J12 * cc[5];
    f.c00 = q0[0] * f.J00 + q0[2] * f.J02;
    f.c01 = q0[1] * f.J11 + q0[2] * f.J12;
    f.c11 = q1[1] * f.J11 + q1[2] * f.J12;
  }
  return conic_of_cov2d(eps2d, f);
}

__device__ __forceinline__ int radius_of(const Fwd &f, int width, int height, float radius_clip) {
#pragma clang fp contract(off)
  const float bh = 0.5f * (f.b00 + f.b11);
  const float v1 = bh + sqrtf(fmaxf(0.01f, bh * bh - f.det1));
  const float radius = ceilf(3.f * sqrtf(v1));
  if (radius <= radius_clip) return 0;
  if (f.u + radius <= 0.f || f.u - radius >= (float)width || f.v + radius <= 0.f ||
      f.v - radius >= (float)height)
    return 0;
  return (int)radius;
}

// ---------------------------------------------------------------------------------------------
struct AdamK {
  float step_size[4];    // lr_k / (1 - beta1^t_k), means | scales | quats | opacities
  float inv_bc2_sqrt[4]; // 1 / sqrt(1 - beta2^t_k)   (each optimizer has its own step count t_k)
  int active[4];         // 0 = this optimizer does not step in this call
  float b1, omb1, b2, omb2, eps;
};

// torch.optim.Adam's update (train_utils.py:50-60: no weight decay, no amsgrad), in torch's order:
//   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= step_size * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// The square root and the quotient use the hardware's 1-ulp v_sqrt_f32 / v_rcp_f32 (and the bias correction is a
// product with the reciprocal formed in double on the host): the correctly rounded forms expand to ~11 instructions
// each -- 33 expansions per Gaussian, a seventh of the projection-backward kernel's dependent instruction stream --
// and the difference, <= 3 ulp of one update, is four orders of magnitude inside the 1e-4 the path is held to.
// (sqrt of a denormal v reads as 0: the denominator is then eps, as it is to within 1e-11 with the exact root.)
__device__ __forceinline__ void adam1(float &p, float g, float &m, float &v, int grp, const AdamK &h) {
#pragma clang fp contract(off)  // (one rounding sequence in every kernel: see forward_geom)
  if (!h.active[grp]) return;
  m = m * h.b1 + g * h.omb1;
  v = v * h.b2 + (g * g) * h.omb2;
  const float denom = __builtin_amdgcn_sqrtf(v) * h.inv_bc2_sqrt[grp] + h.eps;
  p = p - h.step_size[grp] * (m * __builtin_amdgcn_rcpf(denom));
}

struct Grads {
  float mean[3], quat[4], scale[3], opac;
};

// The steps of the reverse sweep that both shape forms share (backward_geom below, covar_pair_vjp in csrc/covar_dev.h).
// conic = B^-1  =>  G = -A V A with V = [[va, vb/2],[vb/2, vc]] (b is stored once): the cotangent of cov2d
__device__ __forceinline__ void conic_vjp(const Fwd &f, float va, float vb, float vc, float &G00, float &G01,
                                          float &G11) {
#pragma clang fp contract(off)
  const float hb = 0.5f * vb;
  const float av00 = f.a * va + f.b * hb, av01 = f.a * hb + f.b * vc;
  const float av10 = f.b * va + f.c * hb, av11 = f.b * hb + f.c * vc;
  G00 = -(av00 * f.a + av01 * f.b);
  G01 = -(av00 * f.b + av01 * f.c);
  G11 = -(av10 * f.b + av11 * f.c);
}

// the compensation's share of G: d comp / d cov2d = (1/(2 comp)) * ((1 - comp^2) conic - eps det(conic) I); gsplat
// guards the division with +1e-6 and the oracle does the same.  DET_GUARD (the covariance form): nothing where the
// determinant ratio is negative (comp is clamped to 0 there).
template <bool DET_GUARD>
__device__ __forceinline__ void comp_vjp(const Fwd &f, float eps2d, float v_comp, float &G00, float &G01, float &G11) {
#pragma clang fp contract(off)
  const float det_conic = f.a * f.c - f.b * f.b;
  const float vs = (!DET_GUARD || f.det0 / f.det1 >= 0.f) ? v_comp * 0.5f / (f.comp + 1e-6f) : 0.f;
  const float omc = 1.f - f.comp * f.comp;
  G00 += vs * (omc * f.a - eps2d * det_conic);
  G01 += vs * (omc * f.b);
  G11 += vs * (omc * f.c - eps2d * det_conic);
}

// camera-space mean's cotangent (vtx, vty, vtz): through mean2d (vx, vy), the depth and -- pinhole -- through J, whose
// cotangents the caller formed (the fov clamp freezes tx = +-lim z).  Ortho: J is constant, the vJ are not read.
template <int CM>
__device__ __forceinline__ void camera_mean_vjp(const Cam &cam, const Fwd &f, float vx, float vy, float v_depth,
                                                float vJ00, float vJ02, float vJ11, float vJ12, float &vtx, float &vty,
                                                float &vtz) {
#pragma clang fp contract(off)
  if constexpr (CM == kOrtho) {
    vtx = cam.fx * vx;
    vty = cam.fy * vy;
    vtz = v_depth;
  } else {
    const float rz3 = f.rz2 * f.rz;
    vtx = cam.fx * f.rz * vx;
    vty = cam.fy * f.rz * vy;
    vtz = -(cam.fx * f.x * vx + cam.fy * f.y * vy) * f.rz2 + v_depth;
    vtz += -cam.fx * f.rz2 * vJ00 - cam.fy * f.rz2 * vJ11;
    if (f.in_x) { vtx += -cam.fx * f.rz2 * vJ02; vtz += 2.f * cam.fx * f.tx * rz3 * vJ02; }
    else        { vtz += cam.fx * f.tx * rz3 * vJ02; }
    if (f.in_y) { vty += -cam.fy * f.rz2 * vJ12; vtz += 2.f * cam.fy * f.ty * rz3 * vJ12; }
    else        { vtz += cam.fy * f.ty * rz3 * vJ12; }
  }
}

// CAM (csrc/viewmat_grad.hip): the same sweep stops at the camera-space cotangents and leaves the CAMERA's share in
// v_cam[12] -- rows of [v_R | v_tr], v_R[i][j] = v_t[i] mean[j] + sum_k vW[3 i + k] M[j][k] with M = Rq diag(s) (the
// transpose-side product of W = Rv M), v_tr = v_t -- from the world mean `mean`; `o` is not touched.  The default
// instantiation is the function every other kernel inlines, instruction for instruction.
// CM = kOrtho: v_P reaches W through the first two rows only, the camera-space mean receives (fx v_u, fy v_v, v_depth)
// and nothing through J (it is constant); the chain from vW and (vtx, vty, vtz) on is the shared one.
template <bool CAM = false, int CM = kPinhole>
__device__ __forceinline__ void backward_geom(const Cam &cam, const Fwd &f, float eps2d, uint32_t flags,
                                              const float4 ga, const float4 gb, bool ext, float v_comp_ext,
                                              float v_depth_ext, Grads &o, float *v_cam = nullptr,
                                              const float *mean = nullptr) {
#pragma clang fp contract(off)  // (one rounding sequence in every kernel: see forward_geom)
  const float vx = ga.x, vy = ga.y;
  const float va = gb.x, vb = gb.y, vc = gb.z, vo_eff = gb.w;
  const bool aa = flags & EG_FLAG_ANTIALIASED;

  // o_eff = o * comp (fused mode); in external mode the caller owns that product (gsplat layout:
  // `opacities * compensations` is a torch op between the two autograd nodes)
  float v_o = ext ? 0.f : (aa ? vo_eff * f.comp : vo_eff);
  const float v_comp = ext ? v_comp_ext : (aa ? vo_eff * f.o : 0.f);

  float G00, G01, G11;
  conic_vjp(f, va, vb, vc, G00, G01, G11);
  if (aa) comp_vjp<false>(f, eps2d, v_comp, G00, G01, G11);
  // cov2d = P P^T  =>  v_P = 2 G P
  float vp0[3], vp1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    vp0[k] = 2.f * (G00 * f.p0[k] + G01 * f.p1[k]);
    vp1[k] = 2.f * (G01 * f.p0[k] + G11 * f.p1[k]);
  }
  // P = J W (ortho: the constant J = [[fx, 0, 0], [0, fy, 0]] has no cotangent)
  float vW[9];
  float vJ00 = 0.f, vJ02 = 0.f, vJ11 = 0.f, vJ12 = 0.f;
  if constexpr (CM != kOrtho) {
    vJ00 = vp0[0] * f.W[0] + vp0[1] * f.W[1] + vp0[2] * f.W[2];
    vJ02 = vp0[0] * f.W[6] + vp0[1] * f.W[7] + vp0[2] * f.W[8];
    vJ11 = vp1[0] * f.W[3] + vp1[1] * f.W[4] + vp1[2] * f.W[5];
    vJ12 = vp1[0] * f.W[6] + vp1[1] * f.W[7] + vp1[2] * f.W[8];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    vW[k] = f.J00 * vp0[k];
    vW[3 + k] = f.J11 * vp1[k];
    if constexpr (CM == kOrtho) vW[6 + k] = 0.f; else vW[6 + k] = f.J02 * vp0[k] + f.J12 * vp1[k];
  }
  float vtx, vty, vtz;
  camera_mean_vjp<CM>(cam, f, vx, vy, v_depth_ext, vJ00, vJ02, vJ11, vJ12, vtx, vty, vtz);
  if constexpr (CAM) {
    const float vt[3] = {vtx, vty, vtz};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        v_cam[4 * i + j] = vt[i] * mean[j] + (vW[3 * i] * (f.Rq[3 * j] * f.s[0]) + vW[3 * i + 1] * (f.Rq[3 * j + 1] * f.s[1]) +
                                              vW[3 * i + 2] * (f.Rq[3 * j + 2] * f.s[2]));
      v_cam[4 * i + 3] = vt[i];
    }
    return;
  }
  o.mean[0] = cam.R[0] * vtx + cam.R[3] * vty + cam.R[6] * vtz;
  o.mean[1] = cam.R[1] * vtx + cam.R[4] * vty + cam.R[7] * vtz;
  o.mean[2] = cam.R[2] * vtx + cam.R[5] * vty + cam.R[8] * vtz;

  // W = Rv M, M = Rq diag(s)
  float vR[9];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float vs = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float vM = cam.R[i] * vW[k] + cam.R[3 + i] * vW[3 + k] + cam.R[6 + i] * vW[6 + k];
      vs += f.Rq[3 * i + k] * vM;
      vR[3 * i + k] = vM * f.s[k];
    }
    o.scale[k] = (flags & EG_FLAG_LOG_SCALES) ? vs * f.s[k] : vs;
  }
  // rotation -> normalised quaternion -> raw quaternion
  const float w = f.qw, x = f.qx, y = f.qy, z = f.qz;
  const float nw = 2.f * (x * (vR[7] - vR[5]) + y * (vR[2] - vR[6]) + z * (vR[3] - vR[1]));
  const float nx = 2.f * (-2.f * x * (vR[4] + vR[8]) + y * (vR[1] + vR[3]) + z * (vR[2] + vR[6]) + w * (vR[7] - vR[5]));
  const float ny = 2.f * (x * (vR[1] + vR[3]) - 2.f * y * (vR[0] + vR[8]) + z * (vR[5] + vR[7]) + w * (vR[2] - vR[6]));
  const float nz = 2.f * (x * (vR[2] + vR[6]) + y * (vR[5] + vR[7]) - 2.f * z * (vR[0] + vR[4]) + w * (vR[3] - vR[1]));
  const float d = nw * w + nx * x + ny * y + nz * z;
  o.quat[0] = (nw - d * w) * f.qinv;
  o.quat[1] = (nx - d * x) * f.qinv;
  o.quat[2] = (ny - d * y) * f.qinv;
  o.quat[3] = (nz - d * z) * f.qinv;

  if (flags & EG_FLAG_LOGIT_OPACITIES) v_o *= f.o * (1.f - f.o);
  o.opac = v_o;
}

// ---------------------------------------------------------------------------------------------
// The quats + scales form of a Gaussian's shape, as the kernels written once for both forms take it (packed.hip,
// viewmat_grad.hip; CovarForm in csrc/covar_dev.h is the other): the inputs, the forward of one (camera, Gaussian)
// pair, the record's opacity, the gradient of one row and the pair's reverse sweep.  The host fills the four pointers;
// `raw` is the kernel's (forward() loads it, pair_vjp reads it).
struct QuatScaleForm {
  const float *means, *quats, *scales, *opacities;
  Raw raw;

  using Visible = float4;  // the dense layout's [C, N, 8] record of the compositing kernels: word 7 is the radius
  static __device__ __forceinline__ bool visible(const float4 *splat, long long q) {
    return __float_as_int(splat[2 * q + 1].w) > 0;
  }

  template <int CM>
  __device__ __forceinline__ bool forward(const Cam &cam, int g, int width, int height, float near_plane,
                                          float far_plane, float eps2d, uint32_t flags, Fwd &f) {
    raw = load_raw(means, quats, scales, opacities, g);
    return forward_geom<CM>(cam, raw, width, height, near_plane, far_plane, eps2d, flags, f);
  }
  __device__ __forceinline__ float opacity(const Fwd &f, int) const { return f.o; }

  // one row of v_means [*, 3], v_quats [*, 4], v_scales [*, 3] (no opacity gradient: the caller owns that product)
  struct Out {
    float *v_means, *v_quats, *v_scales;
  };
  struct Grad : Grads {
    __device__ __forceinline__ void zero() {
#pragma unroll
      for (int k = 0; k < 3; ++k) mean[k] = scale[k] = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) quat[k] = 0.f;
    }
    __device__ __forceinline__ void operator+=(const Grad &o) {
#pragma clang fp contract(off)
#pragma unroll
      for (int k = 0; k < 3; ++k) { mean[k] += o.mean[k]; scale[k] += o.scale[k]; }
#pragma unroll
      for (int k = 0; k < 4; ++k) quat[k] += o.quat[k];
    }
    __device__ __forceinline__ void store(const Out &out, long long row) const {
#pragma unroll
      for (int k = 0; k < 3; ++k) { out.v_means[3 * row + k] = mean[k]; out.v_scales[3 * row + k] = scale[k]; }
#pragma unroll
      for (int k = 0; k < 4; ++k) out.v_quats[4 * row + k] = quat[k];
    }
  };

  // pair p = (cam, g) of a visible list: its share of the row's gradient, or (CAM) the camera's share in v_cam[12].
  // The pair passed the near / far and det culls in the forward, so the recomputation runs with open limits.
  template <bool CAM, int CM>
  __device__ __forceinline__ void pair_vjp(const Cam &cam, int g, long long p, int width, int height, float eps2d,
                                           uint32_t flags, const float4 *__restrict__ g2d,
                                           const float *__restrict__ v_comps, const float *__restrict__ v_depths,
                                           Grad &gr, float *v_cam = nullptr) {
    const float4 ga = g2d[2 * p], gb = g2d[2 * p + 1];
    Fwd f;
    forward<CM>(cam, g, width, height, -3.0e38f, 3.0e38f, eps2d, flags, f);
    backward_geom<CAM, CM>(cam, f, eps2d, flags, ga, gb, true, v_comps[p], v_depths ? v_depths[p] : 0.f, gr, v_cam, raw.m);
  }
};

inline AdamK make_adamk(const eg_adam_hyper &h) {
  // host side in double, exactly how torch.optim.Adam forms its scalars before casting to fp32
  AdamK k;
  const double b1 = h.beta1, b2 = h.beta2;
  const double lrs[4] = {h.lr_means, h.lr_scales, h.lr_quats, h.lr_opacities};
  for (int i = 0; i < 4; ++i) {
    const int t = h.group_steps[i] == 0 ? h.step : h.group_steps[i];  // 0: shared count, < 0: skip
    k.active[i] = t > 0;
    const double tt = t > 0 ? (double)t : 1.0;
    k.step_size[i] = (float)(lrs[i] / (1.0 - pow(b1, tt)));
    k.inv_bc2_sqrt[i] = (float)(1.0 / sqrt(1.0 - pow(b2, tt)));
  }
  k.b1 = (float)b1; k.omb1 = (float)(1.0 - b1);
  k.b2 = (float)b2; k.omb2 = (float)(1.0 - b2);
  k.eps = (float)h.eps;
  return k;
}

}  // namespace eg
