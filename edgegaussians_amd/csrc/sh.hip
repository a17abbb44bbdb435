// Spherical-harmonics colours (gsplat 1.0.0 `spherical_harmonics`, degrees 0..4) and their backward.
//
//   colors[c, n, :] = sum_{k < (L+1)^2} Y_k(dir[c, n] / |dir[c, n]|) * coeffs[(c,) n, k, :]      (+ 0.5, clamped at 0, on request)
//
// Y_k: the real spherical harmonics in Cartesian form times (-1)^m, k = l*l + l + m (the 3DGS / gsplat convention).
// dir[c, n] is given ([C, N, 3]) or formed as means[n] - campos[c].
//
// Mapping: one lane per Gaussian, the C cameras in a loop inside the lane, so that coefficients shared by the cameras are
// read once and their gradient is summed in registers and stored once: no atomics, the same bits on every run.
// Memory: a lane's coefficient row is 3 K contiguous floats (up to 300 bytes), so lane-strided loads would use 4 bytes of
// every line they touch.  The rows of a workgroup's kBlock Gaussians form ONE contiguous span: it is staged through LDS
// with coalesced 16-byte loads (4-byte ones when K is larger than the degree needs -- only the used columns are read --
// or the span is not 16-byte aligned), and the v_coeffs span leaves the same way.  The LDS row stride is 3 (L+1)^2
// rounded up to odd: the 32 lanes of a ds_read_b32 group then fall on 32 different banks (3 K = 12 or 48 would put
// them on 8 or 2).
#include "common.h"

using namespace eg;

namespace {

constexpr int kBlock = 128;

// value + gradient with respect to the (normalised) direction: the backward evaluates the basis ONCE on these and reads
// both the values (for v_coeffs and the clamp gate) and the direction gradient off the result
struct Dual {
  float v, x, y, z;
};
__device__ __forceinline__ Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ Dual operator*(Dual a, Dual b) {
  return {a.v * b.v, a.v * b.x + a.x * b.v, a.v * b.y + a.y * b.v, a.v * b.z + a.z * b.v};
}
__device__ __forceinline__ Dual operator*(float s, Dual a) { return {s * a.v, s * a.x, s * a.y, s * a.z}; }
template <class T> __device__ __forceinline__ T constant(float c);
template <> __device__ __forceinline__ float constant<float>(float c) { return c; }
template <> __device__ __forceinline__ Dual constant<Dual>(float c) { return {c, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ float value(float a) { return a; }
__device__ __forceinline__ float value(Dual a) { return a.v; }

// Y[0 .. (L+1)^2) at the unit vector (x, y, z), every band as a homogeneous polynomial of its degree
template <int L, class T>
__device__ __forceinline__ void sh_basis(T x, T y, T z, T *Y) {
  Y[0] = constant<T>(0.28209479177387814f);
  if constexpr (L >= 1) {
    constexpr float c1 = 0.4886025119029199f;
    Y[1] = -c1 * y;
    Y[2] = c1 * z;
    Y[3] = -c1 * x;
  }
  if constexpr (L >= 2) {
    const T xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    constexpr float c2 = 1.0925484305920792f;
    Y[4] = c2 * xy;
    Y[5] = -c2 * yz;
    Y[6] = 0.31539156525252005f * (2.f * zz - xx - yy);
    Y[7] = -c2 * xz;
    Y[8] = 0.5462742152960396f * (xx - yy);
    if constexpr (L >= 3) {
      constexpr float c3a = 0.5900435899266435f, c3c = 0.4570457994644658f;
      const T f = 4.f * zz - xx - yy;
      Y[9] = -c3a * (y * (3.f * xx - yy));
      Y[10] = 2.890611442640554f * (xy * z);
      Y[11] = -c3c * (y * f);
      Y[12] = 0.3731763325901154f * (z * (2.f * zz - 3.f * xx - 3.f * yy));
      Y[13] = -c3c * (x * f);
      Y[14] = 1.445305721320277f * (z * (xx - yy));
      Y[15] = -c3a * (x * (xx - 3.f * yy));
    }
    if constexpr (L >= 4) {
      constexpr float c4b = 1.7701307697799304f, c4d = 0.6690465435572892f;
      const T r2 = xx + yy + zz;
      const T a = 7.f * zz - r2, b = 7.f * zz - 3.f * r2;
      const T p = xx - 3.f * yy, q = 3.f * xx - yy;
      Y[16] = 2.5033429417967046f * (xy * (xx - yy));
      Y[17] = -c4b * (yz * q);
      Y[18] = 0.9461746957575601f * (xy * a);
      Y[19] = -c4d * (yz * b);
      Y[20] = 0.10578554691520431f * (35.f * (zz * zz) - 30.f * (zz * r2) + 3.f * (r2 * r2));
      Y[21] = -c4d * (xz * b);
      Y[22] = 0.47308734787878004f * ((xx - yy) * a);
      Y[23] = -c4b * (xz * p);
      Y[24] = 0.6258357354491761f * (xx * p - yy * q);
    }
  }
}

// The coefficient rows of `rows` consecutive Gaussians (row pitch K3 = 3 K floats in memory, the first KU3 = 3 (L+1)^2
// of each used) -> LDS rows of pitch STRIDE.
template <int KU3, int STRIDE>
__device__ __forceinline__ void stage_in(float *lds, const float *__restrict__ g, int rows, int K3) {
  const int tid = threadIdx.x;
  if (K3 == KU3 && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {  // the span is dense: 16 bytes per lane
    const int total = rows * KU3, n4 = total >> 2;
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    for (int i = tid; i < n4; i += kBlock) {
      const float4 v = g4[i];
      const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int idx = 4 * i + j, r = idx / KU3;
        lds[r * STRIDE + (idx - r * KU3)] = e[j];
      }
    }
    for (int idx = 4 * n4 + tid; idx < total; idx += kBlock) {
      const int r = idx / KU3;
      lds[r * STRIDE + (idx - r * KU3)] = g[idx];
    }
  } else {
    const int total = rows * KU3;
    for (int idx = tid; idx < total; idx += kBlock) {
      const int r = idx / KU3, col = idx - r * KU3;
      lds[r * STRIDE + col] = g[(size_t)r * K3 + col];
    }
  }
}

// LDS rows -> the v_coeffs rows of `rows` consecutive Gaussians; the columns above the degree's get zeros
template <int KU3, int STRIDE>
__device__ __forceinline__ void stage_out(const float *lds, float *__restrict__ g, int rows, int K3) {
  const int tid = threadIdx.x;
  if (K3 == KU3 && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    const int total = rows * KU3, n4 = total >> 2;
    float4 *g4 = reinterpret_cast<float4 *>(g);
    for (int i = tid; i < n4; i += kBlock) {
      float e[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int idx = 4 * i + j, r = idx / KU3;
        e[j] = lds[r * STRIDE + (idx - r * KU3)];
      }
      g4[i] = make_float4(e[0], e[1], e[2], e[3]);
    }
    for (int idx = 4 * n4 + tid; idx < total; idx += kBlock) {
      const int r = idx / KU3;
      g[idx] = lds[r * STRIDE + (idx - r * KU3)];
    }
  } else {
    const int total = rows * K3;  // (rows <= kBlock, K3 < 2^24: checked by the entry)
    for (int idx = tid; idx < total; idx += kBlock) {
      const int r = idx / K3, col = idx - r * K3;
      g[idx] = col < KU3 ? lds[r * STRIDE + col] : 0.f;
    }
  }
}

struct ShArgs {
  int32_t K, C, N, per_camera, clamp;
  const float *dirs, *means, *campos, *coeffs;
  const uint8_t *masks;
};

// the direction of (camera c, Gaussian n), normalised (a zero vector stays zero), and 1 / its length
__device__ __forceinline__ void unit_dir(const ShArgs &a, int c, size_t i, const float *m, float &x, float &y, float &z,
                                         float &inv) {
  float dx, dy, dz;
  if (a.dirs) {
    dx = a.dirs[3 * i], dy = a.dirs[3 * i + 1], dz = a.dirs[3 * i + 2];
  } else {
    dx = m[0] - a.campos[3 * c], dy = m[1] - a.campos[3 * c + 1], dz = m[2] - a.campos[3 * c + 2];
  }
  const float len = sqrtf(dx * dx + dy * dy + dz * dz);
  inv = len > 0.f ? 1.f / len : 0.f;
  x = dx * inv, y = dy * inv, z = dz * inv;
}

template <int L>
__global__ void __launch_bounds__(kBlock) sh_fwd_kernel(ShArgs a, float *__restrict__ colors) {
  constexpr int KU = (L + 1) * (L + 1), KU3 = 3 * KU, STRIDE = KU3 | 1;
  __shared__ float lds[kBlock * STRIDE];
  const int tid = threadIdx.x;
  const size_t n0 = (size_t)blockIdx.x * kBlock;
  const int rows = (int)min((size_t)kBlock, (size_t)a.N - n0);
  const size_t n = n0 + tid;
  const bool active = tid < rows;
  const int K3 = 3 * a.K;
  float m[3] = {0.f, 0.f, 0.f};
  if (active && !a.dirs) m[0] = a.means[3 * n], m[1] = a.means[3 * n + 1], m[2] = a.means[3 * n + 2];
  const float *row = lds + tid * STRIDE;
  const int sets = a.per_camera ? a.C : 1;
  for (int s = 0; s < sets; ++s) {
    if (s) __syncthreads();
    stage_in<KU3, STRIDE>(lds, a.coeffs + ((size_t)s * a.N + n0) * K3, rows, K3);
    __syncthreads();
    if (!active) continue;
    const int c_end = a.per_camera ? s + 1 : a.C;
    for (int c = a.per_camera ? s : 0; c < c_end; ++c) {
      const size_t i = (size_t)c * a.N + n;
      float r[3] = {0.f, 0.f, 0.f};
      if (!a.masks || a.masks[i]) {
        float x, y, z, inv, Y[KU];
        unit_dir(a, c, i, m, x, y, z, inv);
        sh_basis<L, float>(x, y, z, Y);
#pragma unroll
        for (int k = 0; k < KU; ++k) {
          r[0] += Y[k] * row[3 * k], r[1] += Y[k] * row[3 * k + 1], r[2] += Y[k] * row[3 * k + 2];
        }
        if (a.clamp) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) r[ch] = fmaxf(r[ch] + 0.5f, 0.f);
        }
      }
      colors[3 * i] = r[0], colors[3 * i + 1] = r[1], colors[3 * i + 2] = r[2];
    }
  }
}

template <int L>
__global__ void __launch_bounds__(kBlock) sh_bwd_kernel(ShArgs a, const float *__restrict__ v_colors,
                                                        float *__restrict__ v_coeffs, float *__restrict__ v_dirs,
                                                        float *__restrict__ v_means) {
  constexpr int KU = (L + 1) * (L + 1), KU3 = 3 * KU, STRIDE = KU3 | 1;
  __shared__ float lds[kBlock * STRIDE];
  const int tid = threadIdx.x;
  const size_t n0 = (size_t)blockIdx.x * kBlock;
  const int rows = (int)min((size_t)kBlock, (size_t)a.N - n0);
  const size_t n = n0 + tid;
  const bool active = tid < rows;
  const int K3 = 3 * a.K;
  const bool want_dir = v_dirs || v_means;
  float m[3] = {0.f, 0.f, 0.f};
  if (active && !a.dirs) m[0] = a.means[3 * n], m[1] = a.means[3 * n + 1], m[2] = a.means[3 * n + 2];
  float *row = lds + tid * STRIDE;
  float acc[KU3];
#pragma unroll
  for (int j = 0; j < KU3; ++j) acc[j] = 0.f;
  float vm[3] = {0.f, 0.f, 0.f};
  const int sets = a.per_camera ? a.C : 1;
  for (int s = 0; s < sets; ++s) {
    if (s) __syncthreads();  // (the store of the camera before has read the LDS rows)
    stage_in<KU3, STRIDE>(lds, a.coeffs + ((size_t)s * a.N + n0) * K3, rows, K3);
    __syncthreads();
    if (active) {
      const int c_end = a.per_camera ? s + 1 : a.C;
      for (int c = a.per_camera ? s : 0; c < c_end; ++c) {
        const size_t i = (size_t)c * a.N + n;
        float g[3] = {0.f, 0.f, 0.f};  // dL/d(direction as given)
        if (!a.masks || a.masks[i]) {
          float x, y, z, inv;
          unit_dir(a, c, i, m, x, y, z, inv);
          Dual Y[KU];
          sh_basis<L, Dual>(Dual{x, 1.f, 0.f, 0.f}, Dual{y, 0.f, 1.f, 0.f}, Dual{z, 0.f, 0.f, 1.f}, Y);
          float v[3] = {v_colors[3 * i], v_colors[3 * i + 1], v_colors[3 * i + 2]};
          if (a.clamp) {  // the gate of clamp_min(raw + 0.5, 0), recomputed: gradient passes where raw + 0.5 >= 0
            float r[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < KU; ++k) {
              r[0] += Y[k].v * row[3 * k], r[1] += Y[k].v * row[3 * k + 1], r[2] += Y[k].v * row[3 * k + 2];
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[ch] = (r[ch] + 0.5f >= 0.f) ? v[ch] : 0.f;
          }
          float gd[3] = {0.f, 0.f, 0.f};  // dL/d(unit direction)
#pragma unroll
          for (int k = 0; k < KU; ++k) {
            acc[3 * k] += Y[k].v * v[0], acc[3 * k + 1] += Y[k].v * v[1], acc[3 * k + 2] += Y[k].v * v[2];
            if (want_dir) {
              const float w = row[3 * k] * v[0] + row[3 * k + 1] * v[1] + row[3 * k + 2] * v[2];
              gd[0] += Y[k].x * w, gd[1] += Y[k].y * w, gd[2] += Y[k].z * w;
            }
          }
          // through d = dir / |dir|: (I - d d^T) gd / |dir|
          const float dot = x * gd[0] + y * gd[1] + z * gd[2];
          g[0] = (gd[0] - x * dot) * inv, g[1] = (gd[1] - y * dot) * inv, g[2] = (gd[2] - z * dot) * inv;
        }
        if (v_dirs) v_dirs[3 * i] = g[0], v_dirs[3 * i + 1] = g[1], v_dirs[3 * i + 2] = g[2];
        vm[0] += g[0], vm[1] += g[1], vm[2] += g[2];
      }
    }
    __syncthreads();  // every lane has read its coefficient row: the rows now carry the gradient out
    if (active) {
#pragma unroll
      for (int j = 0; j < KU3; ++j) {
        row[j] = acc[j];
        acc[j] = 0.f;
      }
    }
    __syncthreads();
    stage_out<KU3, STRIDE>(lds, v_coeffs + ((size_t)s * a.N + n0) * K3, rows, K3);
  }
  if (active && v_means) v_means[3 * n] = vm[0], v_means[3 * n + 1] = vm[1], v_means[3 * n + 2] = vm[2];
}

// the checks both entries share; `dirs` given: directions as they are, else means - campos
#define EG_SH_CHECK()                                                                                            \
  do {                                                                                                           \
    EG_REQUIRE(degree >= 0 && degree <= 4, "degree must be 0..4");                                               \
    EG_REQUIRE(C >= 1 && N >= 0, "bad sizes (C >= 1, N >= 0)");                                                  \
    EG_REQUIRE(K >= (degree + 1) * (degree + 1) && K <= (1 << 16), "K must be (degree + 1)^2 .. 65536");         \
    EG_REQUIRE(coeffs_per_camera == 0 || coeffs_per_camera == 1, "coeffs_per_camera must be 0 or 1");            \
    EG_REQUIRE(coeffs, "null coeffs");                                                                           \
    EG_REQUIRE(dirs || (means && campos), "null directions: dirs, or means and campos");                         \
    EG_REQUIRE(!dirs || (!means && !campos), "dirs and means / campos are exclusive");                           \
  } while (0)

#define EG_SH_DISPATCH(KERNEL, ...)                                                              \
  do {                                                                                           \
    const dim3 grid(cdiv(N, kBlock));                                                            \
    switch (degree) {                                                                            \
      case 0: KERNEL<0><<<grid, kBlock, 0, s>>>(__VA_ARGS__); break;                             \
      case 1: KERNEL<1><<<grid, kBlock, 0, s>>>(__VA_ARGS__); break;                             \
      case 2: KERNEL<2><<<grid, kBlock, 0, s>>>(__VA_ARGS__); break;                             \
      case 3: KERNEL<3><<<grid, kBlock, 0, s>>>(__VA_ARGS__); break;                             \
      default: KERNEL<4><<<grid, kBlock, 0, s>>>(__VA_ARGS__); break;                            \
    }                                                                                            \
  } while (0)

}  // namespace

extern "C" int eg_sh_fwd(int32_t degree, int32_t K, int32_t C, int32_t N, const float *dirs, const float *means,
                         const float *campos, const float *coeffs, int32_t coeffs_per_camera, const uint8_t *masks,
                         int32_t clamp, float *colors, eg_stream_t stream) {
  EG_SH_CHECK();
  EG_REQUIRE(colors, "null colors");
  if (N == 0) return EG_OK;
  const ShArgs a = {K, C, N, coeffs_per_camera, clamp != 0, dirs, means, campos, coeffs, masks};
  hipStream_t s = as_stream(stream);
  EG_SH_DISPATCH(sh_fwd_kernel, a, colors);
  return check_launch("sh_fwd");
}

extern "C" int eg_sh_bwd(int32_t degree, int32_t K, int32_t C, int32_t N, const float *dirs, const float *means,
                         const float *campos, const float *coeffs, int32_t coeffs_per_camera, const uint8_t *masks,
                         int32_t clamp, const float *v_colors, float *v_coeffs, float *v_dirs, float *v_means,
                         eg_stream_t stream) {
  EG_SH_CHECK();
  EG_REQUIRE(v_colors && v_coeffs, "null v_colors / v_coeffs");
  EG_REQUIRE(!v_dirs || dirs, "v_dirs goes with dirs");
  EG_REQUIRE(!v_means || means, "v_means goes with means / campos");
  if (N == 0) return EG_OK;
  const ShArgs a = {K, C, N, coeffs_per_camera, clamp != 0, dirs, means, campos, coeffs, masks};
  hipStream_t s = as_stream(stream);
  EG_SH_DISPATCH(sh_bwd_kernel, a, v_colors, v_coeffs, v_dirs, v_means);
  return check_launch("sh_bwd");
}
