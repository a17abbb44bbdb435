// Parametric edges -> points: the sampling step in front of the reference's evaluation
// (eval_utils.py:120-398, get_pred_points_and_directions[_from_dict]) on the device, float64 throughout.
//
//   eg_edge_sample_count: per primitive (all cubic Beziers, then all lines) its length, its sample count
//                         int(length // resolution) and the exclusive scan of the counts
//   eg_edge_sample_emit:  one thread per sample: np.linspace(0, 1, n) parameter, point, direction, primitive id
//   eg_edge_sample:       both, with one read-back of the total in between
//
// The reference's rules are restated, not improved: the curve length is its composite Simpson sum of 100 x 101
// derivative norms, the curve direction of tangent mode 0 is its formula with the extra factors 3 and 2.
// No float atomics: every sum has a fixed order, two runs give the same bits.
#include <math.h>

#include "common.h"

namespace eg {
namespace {

constexpr int kLenThreads = 256;
constexpr int kSimpson = 100;                                // bezier_curve_length(num_samples=100)
constexpr int kSimpsonTerms = kSimpson * (kSimpson + 1);     // 100 sub-intervals x nodes 0..100
constexpr int kScanThreads = 256;

// sum of a double over the wave, in lane 63: the six DPP steps of wave_sum_dpp_f on both halves of the value (lanes a
// step leaves without a source add +0.0)
__device__ __forceinline__ double wave_sum_dpp_d(double x) {
#define EG_DPP_STEPD(ctrl, rmask)                                                                        \
  {                                                                                                      \
    const long long b = __double_as_longlong(x);                                                         \
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(b >> 32), ctrl, rmask, 0xf, false); \
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)b, ctrl, rmask, 0xf, false);        \
    x += __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));                         \
  }
  EG_DPP_STEPD(0x111, 0xf); EG_DPP_STEPD(0x112, 0xf); EG_DPP_STEPD(0x114, 0xf); EG_DPP_STEPD(0x118, 0xf);
  EG_DPP_STEPD(0x142, 0xa); EG_DPP_STEPD(0x143, 0xc);
#undef EG_DPP_STEPD
  return x;
}

// int(length // resolution) as Python and numpy divide floats (CPython float_floor_div, numpy npy_floor_divide): the
// floor of the EXACT quotient -- fmod is exact, (a - mod) / b is then within an ulp of an integer, and the half
// correction puts it on that integer.  floor(a / b) is not the same: 0.1 / 0.02 rounds up to 5.0, 0.1 // 0.02 is 4.
// a >= 0, b > 0 here.  Saturates at INT32_MAX (the scan then reports the overflow).
__device__ __forceinline__ int floor_div_count(double a, double b) {
#pragma clang fp contract(off)
  const double mod = fmod(a, b);
  const double div = (a - mod) / b;  // (mod has a's sign, b > 0: no sign fix-up)
  if (!(div > 0.0)) return 0;
  double fl = floor(div);
  if (div - fl > 0.5) fl += 1.0;
  return fl >= 2147483647.0 ? 2147483647 : (int)fl;
}

// One workgroup per curve.  Term e = 101 i + j is node j of sub-interval [i / 100, (i + 1) / 100]:
//   |B'(a + j h)| (j < 100) or |B'(b)| (j = 100), weight 1 4 2 4 ... 2 4 1, times h = (b - a) / 100;  length = sum / 3.
// Lane `tid` takes the terms tid, tid + 256, ... in that order; then the wave reduction, then the tree over the four
// wave sums in LDS.
__global__ void __launch_bounds__(kLenThreads)
edge_curve_length_kernel(const double *__restrict__ curves, int Nc, double resolution, double *__restrict__ lengths,
                         int *__restrict__ counts) {
  __shared__ double wave_sum[kLenThreads / 64];
  const int c = blockIdx.x, tid = threadIdx.x;
  if (c >= Nc) return;
  const double *P = curves + (size_t)c * 12;
  double d0[3], d1[3], d2[3];  // the differences the derivative weighs (eval_utils.py:124-135), times n = 3
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    d0[a] = P[3 + a] - P[a];
    d1[a] = P[6 + a] - P[3 + a];
    d2[a] = P[9 + a] - P[6 + a];
  }
  double acc = 0.0;
  for (int e = tid; e < kSimpsonTerms; e += kLenThreads) {
    const int i = e / (kSimpson + 1), j = e - i * (kSimpson + 1);
    const double a = (double)i / kSimpson, b = (double)(i + 1) / kSimpson;
    const double h = (b - a) / kSimpson;
    const double t = j == kSimpson ? b : a + j * h;
    const double u = 1.0 - t;
    const double w0 = 3.0 * (u * u), w1 = 3.0 * 2.0 * u * t, w2 = 3.0 * (t * t);
    const double x = w0 * d0[0] + w1 * d1[0] + w2 * d2[0];
    const double y = w0 * d0[1] + w1 * d1[1] + w2 * d2[1];
    const double z = w0 * d0[2] + w1 * d1[2] + w2 * d2[2];
    const double wt = (j == 0 || j == kSimpson) ? 1.0 : ((j & 1) ? 4.0 : 2.0);
    acc += wt * sqrt(x * x + y * y + z * z) * h;
  }
  acc = wave_sum_dpp_d(acc);
  if ((tid & 63) == 63) wave_sum[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    const double len = ((wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3])) / 3.0;
    lengths[c] = len;
    counts[c] = floor_div_count(len, resolution);
  }
}

// One thread per line: |p0 - p1| and its count, behind the curves
__global__ void __launch_bounds__(kLenThreads)
edge_line_length_kernel(const double *__restrict__ lines, int Nl, double resolution, double *__restrict__ lengths,
                        int *__restrict__ counts) {
  const int l = blockIdx.x * kLenThreads + threadIdx.x;
  if (l >= Nl) return;
  const double *P = lines + (size_t)l * 6;
  const double x = P[0] - P[3], y = P[1] - P[4], z = P[2] - P[5];
  const double len = sqrt(x * x + y * y + z * z);
  lengths[l] = len;
  counts[l] = floor_div_count(len, resolution);
}

// Exclusive scan of the counts by ONE workgroup, a block of kScanThreads primitives per round, the running sum in
// int64.  offsets[P] = total.  A total above `limit` (the caller's capacity, at most INT32_MAX) raises total[1]; the
// offsets are saturated at INT32_MAX then and nothing may be emitted from them.
__global__ void __launch_bounds__(kScanThreads)
edge_count_scan_kernel(const int *__restrict__ counts, int P, long long limit, int *__restrict__ offsets,
                       int *__restrict__ total) {
  __shared__ long long buf[2][kScanThreads];
  const int tid = threadIdx.x;
  long long carry = 0;
  for (int base = 0; base < P; base += kScanThreads) {
    const int p = base + tid;
    const long long c = p < P ? (long long)counts[p] : 0;
    int cur = 0;
    buf[0][tid] = c;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {  // (inclusive, Hillis-Steele: integers, any order gives the same sum)
      const long long v = buf[cur][tid] + (tid >= d ? buf[cur][tid - d] : 0);
      buf[cur ^ 1][tid] = v;
      cur ^= 1;
      __syncthreads();
    }
    const long long excl = carry + buf[cur][tid] - c;
    if (p < P) offsets[p] = excl > 2147483647ll ? 2147483647 : (int)excl;
    carry += buf[cur][kScanThreads - 1];
    __syncthreads();
  }
  if (tid == 0) {
    const int sat = carry > 2147483647ll ? 2147483647 : (int)carry;
    offsets[P] = sat;
    total[0] = sat;
    total[1] = carry > limit ? 1 : 0;
  }
}

// One thread per sample.  Nothing is written when the scan raised the overflow flag, beyond total[0] or beyond
// `capacity` rows.
template <bool EXACT_TANGENT>
__global__ void __launch_bounds__(256)
edge_emit_kernel(const double *__restrict__ curves, int Nc, const double *__restrict__ lines, int Nl,
                 const int *__restrict__ counts, const int *__restrict__ offsets, const int *__restrict__ total,
                 long long capacity, float *__restrict__ points, float *__restrict__ directions,
                 int *__restrict__ prim_ids) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (total[1] != 0 || i >= total[0] || i >= capacity) return;
  // the primitive: the last p with offsets[p] <= i (primitives without samples share their successor's offset)
  int lo = 0, hi = Nc + Nl;  // offsets[lo] <= i < offsets[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= (int)i) lo = mid; else hi = mid;
  }
  const int p = lo, n = counts[p], k = (int)i - offsets[p];
  // np.linspace(0, 1, n): k * (1 / (n - 1)), the last sample exactly 1; n == 1: 0
  const double step = 1.0 / (double)(n - 1);
  const double t = n == 1 ? 0.0 : (k == n - 1 ? 1.0 : (double)k * step);
  double pt[3], dir[3];
  if (p < Nc) {
    const double *P = curves + (size_t)p * 12;
    const double t2 = t * t, t3 = t2 * t;
    // [t^3 t^2 t 1] . M, M = [[-1 3 -3 1] [3 -6 3 0] [-3 3 0 0] [1 0 0 0]] (eval_utils.py:312-314)
    const double c0 = -t3 + 3.0 * t2 - 3.0 * t + 1.0, c1 = 3.0 * t3 - 6.0 * t2 + 3.0 * t, c2 = -3.0 * t3 + 3.0 * t2, c3 = t3;
    // direction: A u + B v + C with A = -3 P0 + 9 P1 - 9 P2 + 3 P3, B = 6 P0 - 12 P1 + 6 P2, C = -3 P0 + 3 P1.  The true
    // derivative has u = t^2, v = t; the reference writes u = 3 t^2, v = 2 t (eval_utils.py:323-324)
    const double u = EXACT_TANGENT ? t2 : 3.0 * t2, v = EXACT_TANGENT ? t : 2.0 * t;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double p0 = P[a], p1 = P[3 + a], p2 = P[6 + a], p3 = P[9 + a];
      pt[a] = c0 * p0 + c1 * p1 + c2 * p2 + c3 * p3;
      dir[a] = (-3.0 * p0 + 9.0 * p1 - 9.0 * p2 + 3.0 * p3) * u + (6.0 * p0 - 12.0 * p1 + 6.0 * p2) * v +
               (-3.0 * p0 + 3.0 * p1);
    }
    const double nrm = sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);  // (0 gives nan, as in the reference)
#pragma unroll
    for (int a = 0; a < 3; ++a) dir[a] = dir[a] / nrm;
  } else {
    const double *P = lines + (size_t)(p - Nc) * 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      pt[a] = (1.0 - t) * P[a] + t * P[3 + a];
      dir[a] = P[3 + a] - P[a];
    }
    const double nrm = sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]) + 1e-6;  // eval_utils.py:389-391
#pragma unroll
    for (int a = 0; a < 3; ++a) dir[a] = dir[a] / nrm;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) points[i * 3 + a] = (float)pt[a];
  if (directions) {
#pragma unroll
    for (int a = 0; a < 3; ++a) directions[i * 3 + a] = (float)dir[a];
  }
  if (prim_ids) prim_ids[i] = p;
}

constexpr int64_t kEdgeMaxPrims = 1ll << 30;  // Nc + Nl + 1 offsets are indexed with 32-bit integers

int launch_count(const double *curves, int32_t Nc, const double *lines, int32_t Nl, double resolution, int64_t capacity,
                 double *lengths, int32_t *counts, int32_t *offsets, int32_t *total, hipStream_t st) {
  if (Nc > 0) edge_curve_length_kernel<<<Nc, kLenThreads, 0, st>>>(curves, Nc, resolution, lengths, counts);
  if (Nl > 0)
    edge_line_length_kernel<<<cdiv(Nl, kLenThreads), kLenThreads, 0, st>>>(lines, Nl, resolution, lengths + Nc,
                                                                          counts + Nc);
  const long long limit = capacity < 0 || capacity > 2147483647ll ? 2147483647ll : capacity;
  edge_count_scan_kernel<<<1, kScanThreads, 0, st>>>(counts, Nc + Nl, limit, offsets, total);
  return check_launch("edge_sample_count");
}

int launch_emit(const double *curves, int32_t Nc, const double *lines, int32_t Nl, const int32_t *counts,
                const int32_t *offsets, const int32_t *total, int64_t capacity, int32_t tangent, float *points,
                float *directions, int32_t *prim_ids, hipStream_t st) {
  const int blocks = cdiv(capacity, 256);
  if (tangent == EG_EDGE_TANGENT_EXACT)
    edge_emit_kernel<true><<<blocks, 256, 0, st>>>(curves, Nc, lines, Nl, counts, offsets, total, capacity, points,
                                                   directions, prim_ids);
  else
    edge_emit_kernel<false><<<blocks, 256, 0, st>>>(curves, Nc, lines, Nl, counts, offsets, total, capacity, points,
                                                    directions, prim_ids);
  return check_launch("edge_sample_emit");
}

}  // namespace
}  // namespace eg

using namespace eg;

#define EG_EDGE_REQUIRE_SIZES()                                                                      \
  EG_REQUIRE(Nc >= 0 && Nl >= 0 && (int64_t)Nc + Nl < kEdgeMaxPrims, "bad sizes (Nc, Nl >= 0, Nc + Nl < 2^30)")

extern "C" int eg_edge_sample_count(const double *curves, int32_t Nc, const double *lines, int32_t Nl, double resolution,
                                    int64_t capacity, double *lengths, int32_t *counts, int32_t *offsets, int32_t *total,
                                    eg_stream_t stream) {
  EG_EDGE_REQUIRE_SIZES();
  EG_REQUIRE(resolution > 0.0 && resolution <= 1.7976931348623157e308, "resolution must be positive and finite");
  EG_REQUIRE((curves || Nc == 0) && (lines || Nl == 0) && offsets && total, "null pointer");
  EG_REQUIRE((lengths && counts) || Nc + Nl == 0, "null pointer");
  return launch_count(curves, Nc, lines, Nl, resolution, capacity, lengths, counts, offsets, total, as_stream(stream));
}

extern "C" int eg_edge_sample_emit(const double *curves, int32_t Nc, const double *lines, int32_t Nl,
                                   const int32_t *counts, const int32_t *offsets, const int32_t *total, int64_t capacity,
                                   int32_t tangent, float *points, float *directions, int32_t *prim_ids,
                                   eg_stream_t stream) {
  EG_EDGE_REQUIRE_SIZES();
  EG_REQUIRE(capacity >= 0 && capacity <= 2147483647ll, "bad capacity (0 <= capacity <= INT32_MAX)");
  EG_REQUIRE(tangent == EG_EDGE_TANGENT_REFERENCE || tangent == EG_EDGE_TANGENT_EXACT, "unknown tangent mode");
  if (capacity == 0 || Nc + Nl == 0) return EG_OK;
  EG_REQUIRE((curves || Nc == 0) && (lines || Nl == 0) && counts && offsets && total && points, "null pointer");
  return launch_emit(curves, Nc, lines, Nl, counts, offsets, total, capacity, tangent, points, directions, prim_ids,
                     as_stream(stream));
}

extern "C" int eg_edge_sample(const double *curves, int32_t Nc, const double *lines, int32_t Nl, double resolution,
                              int64_t capacity, int32_t tangent, double *lengths, int32_t *counts, int32_t *offsets,
                              int32_t *total, float *points, float *directions, int32_t *prim_ids, int32_t *total_host,
                              eg_stream_t stream) {
  EG_EDGE_REQUIRE_SIZES();
  EG_REQUIRE(resolution > 0.0 && resolution <= 1.7976931348623157e308, "resolution must be positive and finite");
  EG_REQUIRE(capacity >= 0 && capacity <= 2147483647ll, "bad capacity (0 <= capacity <= INT32_MAX)");
  EG_REQUIRE(tangent == EG_EDGE_TANGENT_REFERENCE || tangent == EG_EDGE_TANGENT_EXACT, "unknown tangent mode");
  EG_REQUIRE((curves || Nc == 0) && (lines || Nl == 0) && offsets && total && total_host, "null pointer");
  EG_REQUIRE((lengths && counts) || Nc + Nl == 0, "null pointer");
  EG_REQUIRE(points || capacity == 0, "null pointer");
  hipStream_t st = as_stream(stream);
  int rc = launch_count(curves, Nc, lines, Nl, resolution, capacity, lengths, counts, offsets, total, st);
  if (rc) return rc;
  // the one read-back: the total sizes the emission and tells whether it fits
  if (hipMemcpyAsync(total_host, total, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    set_error("eg_edge_sample: reading the total back failed: %s", hipGetErrorString(hipGetLastError()));
    return EG_ERR_LAUNCH;
  }
  if (total_host[1] != 0) {
    set_error("eg_edge_sample: the edges give more samples than the capacity of %lld (or than INT32_MAX)",
              (long long)capacity);
    return EG_ERR_CAPACITY;
  }
  if (total_host[0] == 0) return EG_OK;
  return launch_emit(curves, Nc, lines, Nl, counts, offsets, total, total_host[0], tangent, points, directions, prim_ids,
                     st);
}
