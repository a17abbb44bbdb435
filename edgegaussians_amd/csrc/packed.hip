// Packed projection (gsplat `rasterization(packed=True)`): only the visible (camera, Gaussian) pairs are kept.
//
// The general path writes 17 words for every one of the C * N pairs (csrc/cams.hip, eg_project_fwd_cams).  Here a
// COUNT pass decides the culls and a WRITE pass compacts: pair (c, n) survives exactly when `radius_of` is positive
// after `forward_geom` -- the same two functions with the same arguments as project_fwd_kernel, so the kept set is
// the set radii[c, n] > 0 of the dense call and every kept value is the dense value, bit for bit.  The pairs come in
// ascending order of c * N + n: camera c owns [indptr[c], indptr[c + 1]) and its gaussian_ids ascend.
//
//   count   grid (ceil(N / 256), C): a workgroup never straddles a camera; it writes its number of visible pairs.
//   scan    one workgroup: the C * ceil(N / 256) counts become workgroup bases (in place), indptr [C + 1] on the way.
//   write   the same grid recomputes the projection (~150 flops, cheaper than storing it), ranks the visible threads
//           with ballot / popcount and a 4-wave prefix, and writes the record of the compositing kernels, the per-pair
//           outputs, the ids, tiles_per_gauss and the per-camera tile counters (LDS histogram, one global atomic per
//           workgroup and touched tile, like project_fwd_kernel).
//   bin     camera c's range is a single-camera problem: eg_tile_emit / eg_sort_pairs through base pointers, then
//           the sorted ids are rebased to the whole packed list and the camera goes into the isect ids.
//   bwd     dense gradients: one thread per Gaussian walks the cameras 0 .. C-1 (eg_project_bwd_cams's order), finds
//           its pair by binary search in the camera's ascending ids, sums in registers, writes every row once (zeros
//           where nobody sees it).  No atomics, no zero-fill: bit-identical from run to run.
//           sparse gradients: one thread per pair, no reduction.
//
// Scratch: 4 bytes per 256 pairs (the workgroup counts).  Nothing of size C * N is allocated.
//
// Every pass but scan / bin exists in a second form for covariances (eg_packed_*_covars, below the quats + scales kernels).
#include "common.h"
#include "covar_dev.h"
#include "project_dev.h"

namespace eg {

constexpr int kPk = 256;  // threads (= Gaussians) per workgroup of the count and write passes

// this thread's Gaussian in camera blockIdx.y: radius after every cull (0 = not kept).  CM: the camera model
// (csrc/project_dev.h) of every kernel here, kOrtho with EG_FLAG_ORTHO.
template <int CM>
__device__ __forceinline__ int packed_project(const float *__restrict__ means, const float *__restrict__ quats,
                                              const float *__restrict__ scales, const float *__restrict__ opacities,
                                              const float *__restrict__ viewmats, const float *__restrict__ Ks, int N,
                                              int width, int height, float near_plane, float far_plane, float eps2d,
                                              float radius_clip, uint32_t flags, int g, Fwd &f) {
  if (g >= N) return 0;
  const Cam cam = load_cam(viewmats + 16 * (size_t)blockIdx.y, Ks + 9 * (size_t)blockIdx.y);
  if (!forward_geom<CM>(cam, means, quats, scales, opacities, g, width, height, near_plane, far_plane, eps2d, flags, f))
    return 0;
  return radius_of(f, width, height, radius_clip);
}

template <int CM>
__global__ void __launch_bounds__(kPk)
packed_count_kernel(const float *__restrict__ means, const float *__restrict__ quats, const float *__restrict__ scales,
                    const float *__restrict__ opacities, const float *__restrict__ viewmats,
                    const float *__restrict__ Ks, int N, int width, int height, float near_plane, float far_plane,
                    float eps2d, float radius_clip, uint32_t flags, int *__restrict__ block_counts) {
  __shared__ int s_wave[kPk / 64];
  const int g = blockIdx.x * kPk + threadIdx.x;
  Fwd f;
  const int radius = packed_project<CM>(means, quats, scales, opacities, viewmats, Ks, N, width, height, near_plane,
                                        far_plane, eps2d, radius_clip, flags, g, f);
  const unsigned long long vote = __ballot(radius > 0);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(vote);
  __syncthreads();
  if (threadIdx.x == 0)
    block_counts[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// counts [C * nb] -> exclusive bases (in place, int32: the host checks nnz < 2^31 on indptr), indptr [C + 1] (int64)
__global__ void __launch_bounds__(256)
packed_scan_kernel(int *__restrict__ block_counts, int nb, int C, long long *__restrict__ indptr) {
  __shared__ int s_tmp[4];
  const long long total = (long long)nb * C;
  if (total == 0) {  // (no Gaussians: every range is empty)
    for (int c = threadIdx.x; c <= C; c += 256) indptr[c] = 0;
    return;
  }
  long long carry = 0;
  for (long long i0 = 0; i0 < total; i0 += 256) {
    const long long i = i0 + threadIdx.x;
    const int c = i < total ? block_counts[i] : 0;
    int chunk;
    const int e = block_excl_scan<256>(c, s_tmp, chunk);
    if (i < total) {
      block_counts[i] = (int)(carry + e);
      if (i % nb == 0) indptr[i / nb] = carry + e;  // the first workgroup of a camera
    }
    carry += chunk;
  }
  if (threadIdx.x == 0) indptr[C] = carry;
}

template <bool LDS_COUNT, int CM>
__global__ void __launch_bounds__(kPk)
packed_write_kernel(const float *__restrict__ means, const float *__restrict__ quats, const float *__restrict__ scales,
                    const float *__restrict__ opacities, const float *__restrict__ viewmats,
                    const float *__restrict__ Ks, int N, int width, int height, float near_plane, float far_plane,
                    float eps2d, float radius_clip, uint32_t flags, const int *__restrict__ block_base, long long nnz,
                    float4 *__restrict__ splat, int *__restrict__ radii, float *__restrict__ means2d,
                    float *__restrict__ depths, float *__restrict__ conics, float *__restrict__ comps,
                    int *__restrict__ tiles_per_gauss, long long *__restrict__ camera_ids,
                    long long *__restrict__ gaussian_ids, int *__restrict__ tile_counts) {
  extern __shared__ __attribute__((aligned(16))) int s_hist[];
  __shared__ int s_wave[kPk / 64];
  const int tw = (width + kTile - 1) / kTile, th = (height + kTile - 1) / kTile, T = tw * th;
  tile_counts += (size_t)blockIdx.y * T;
  if (LDS_COUNT) {
    for (int t = threadIdx.x; t < T; t += kPk) s_hist[t] = 0;
  }
  const int g = blockIdx.x * kPk + threadIdx.x;
  Fwd f;
  const int radius = packed_project<CM>(means, quats, scales, opacities, viewmats, Ks, N, width, height, near_plane,
                                        far_plane, eps2d, radius_clip, flags, g, f);
  const bool keep = radius > 0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long vote = __ballot(keep);
  if (lane == 0) s_wave[wv] = __popcll(vote);
  __syncthreads();  // (also: the histogram is zero)
  if (!keep) {
    if (!LDS_COUNT) return;
  } else {
    long long p = block_base[(size_t)blockIdx.y * gridDim.x + blockIdx.x] + __popcll(vote & ((1ull << lane) - 1ull));
    for (int w = 0; w < wv; ++w) p += s_wave[w];
    if (p >= 0 && p < nnz) {  // (always: nnz is the sum the bases were scanned from -- a guard against a caller's stale scratch)
      const bool aa = flags & EG_FLAG_ANTIALIASED;
      splat[2 * p] = make_float4(f.u, f.v, f.a, f.b);
      splat[2 * p + 1] = make_float4(f.c, aa ? f.o * f.comp : f.o, f.z, __int_as_float(radius));
      radii[p] = radius;
      means2d[2 * p] = f.u; means2d[2 * p + 1] = f.v;
      depths[p] = f.z;
      conics[3 * p] = f.a; conics[3 * p + 1] = f.b; conics[3 * p + 2] = f.c;
      comps[p] = f.comp;
      camera_ids[p] = blockIdx.y;
      gaussian_ids[p] = g;
      int x0, y0, x1, y1;
      tile_box(f.u, f.v, radius, tw, th, x0, y0, x1, y1);
      tiles_per_gauss[p] = (y1 - y0) * (x1 - x0);
      for (int ty = y0; ty < y1; ++ty)
        for (int tx = x0; tx < x1; ++tx) atomicAdd(LDS_COUNT ? &s_hist[ty * tw + tx] : &tile_counts[ty * tw + tx], 1);
    }
  }
  if (LDS_COUNT) {
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += kPk) {
      const int c = s_hist[t];
      if (c) atomicAdd(&tile_counts[t], c);
    }
  }
}

// sorted ids of one camera's range -> indices into the whole packed list; the camera into the isect ids
__global__ void __launch_bounds__(256)
packed_rebase_kernel(int *__restrict__ flatten_ids, long long *__restrict__ isect_ids, long long M, int id_base,
                     long long camera_bits) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= M) return;
  flatten_ids[i] += id_base;
  if (isect_ids) isect_ids[i] |= camera_bits;
}

template <int CM>
__device__ __forceinline__ void packed_pair_vjp(const float *__restrict__ means, const float *__restrict__ quats,
                                                const float *__restrict__ scales, const float *__restrict__ opacities,
                                                const float *__restrict__ viewmats, const float *__restrict__ Ks,
                                                int cam_id, int g, long long p, int width, int height, float eps2d,
                                                uint32_t flags, const float4 *__restrict__ g2d,
                                                const float *__restrict__ v_comps, const float *__restrict__ v_depths,
                                                Grads &gr) {
  const Cam cam = load_cam(viewmats + 16 * (size_t)cam_id, Ks + 9 * (size_t)cam_id);
  const float4 ga = g2d[2 * p], gb = g2d[2 * p + 1];
  Fwd f;
  // near / far and det culls already passed in the forward (the pair exists), so pass open limits
  forward_geom<CM>(cam, means, quats, scales, opacities, g, width, height, -3.0e38f, 3.0e38f, eps2d, flags, f);
  backward_geom<false, CM>(cam, f, eps2d, flags, ga, gb, true, v_comps[p], v_depths ? v_depths[p] : 0.f, gr);
}

template <int CM>
__global__ void __launch_bounds__(256)
packed_bwd_dense_kernel(const float *__restrict__ means, const float *__restrict__ quats,
                        const float *__restrict__ scales, const float *__restrict__ opacities,
                        const float *__restrict__ viewmats, const float *__restrict__ Ks, int N, int C, int width,
                        int height, float eps2d, uint32_t flags, const long long *__restrict__ indptr, long long nnz,
                        const long long *__restrict__ gaussian_ids, const float4 *__restrict__ g2d,
                        const float *__restrict__ v_comps, const float *__restrict__ v_depths,
                        float *__restrict__ v_means, float *__restrict__ v_quats, float *__restrict__ v_scales) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= N) return;
  Grads acc;
#pragma unroll
  for (int k = 0; k < 3; ++k) acc.mean[k] = acc.scale[k] = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) acc.quat[k] = 0.f;
  for (int c = 0; c < C; ++c) {
    const long long end = min(indptr[c + 1], nnz);  // (indptr is the scan's: a guard against a caller's stale array)
    long long lo = max(0ll, indptr[c]);
    long long hi = end;
    while (lo < hi) {  // first position whose id is >= g
      const long long mid = lo + ((hi - lo) >> 1);
      if (gaussian_ids[mid] < g) lo = mid + 1; else hi = mid;
    }
    if (lo >= end || gaussian_ids[lo] != g) continue;
    Grads gr;
    packed_pair_vjp<CM>(means, quats, scales, opacities, viewmats, Ks, c, g, lo, width, height, eps2d, flags, g2d, v_comps,
                        v_depths, gr);
#pragma unroll
    for (int k = 0; k < 3; ++k) { acc.mean[k] += gr.mean[k]; acc.scale[k] += gr.scale[k]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) acc.quat[k] += gr.quat[k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) { v_means[3 * g + k] = acc.mean[k]; v_scales[3 * g + k] = acc.scale[k]; }
#pragma unroll
  for (int k = 0; k < 4; ++k) v_quats[4 * g + k] = acc.quat[k];
}

template <int CM>
__global__ void __launch_bounds__(256)
packed_bwd_sparse_kernel(const float *__restrict__ means, const float *__restrict__ quats,
                         const float *__restrict__ scales, const float *__restrict__ opacities,
                         const float *__restrict__ viewmats, const float *__restrict__ Ks, int N, int C, int width,
                         int height, float eps2d, uint32_t flags, long long nnz,
                         const long long *__restrict__ camera_ids, const long long *__restrict__ gaussian_ids,
                         const float4 *__restrict__ g2d, const float *__restrict__ v_comps,
                         const float *__restrict__ v_depths, float *__restrict__ v_means, float *__restrict__ v_quats,
                         float *__restrict__ v_scales) {
  const long long p = blockIdx.x * 256ll + threadIdx.x;
  if (p >= nnz) return;
  const long long c = camera_ids[p], g = gaussian_ids[p];
  Grads gr;
#pragma unroll
  for (int k = 0; k < 3; ++k) gr.mean[k] = gr.scale[k] = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) gr.quat[k] = 0.f;
  if (c >= 0 && c < C && g >= 0 && g < N)  // (ids written by packed_write_kernel: a guard against a caller's stale arrays)
    packed_pair_vjp<CM>(means, quats, scales, opacities, viewmats, Ks, (int)c, (int)g, p, width, height, eps2d, flags, g2d,
                        v_comps, v_depths, gr);
#pragma unroll
  for (int k = 0; k < 3; ++k) { v_means[3 * p + k] = gr.mean[k]; v_scales[3 * p + k] = gr.scale[k]; }
#pragma unroll
  for (int k = 0; k < 4; ++k) v_quats[4 * p + k] = gr.quat[k];
}

// ---------------------------------------------------------------------------------------------
// The covariance form (gsplat `rasterization(covars=[N, 3, 3])`): the world covariance arrives as its upper triangle
// covars [N, 6] instead of quats + scales.  The keep decision is forward_geom_covar + radius_of with the arguments of
// project_covars_fwd_kernel (csrc/functional.hip), so the kept set is the set radii > 0 of eg_project_covars_fwd_cams_flags
// and every kept value is its value, bit for bit.  Same grids, ranking, histogram and order of sums as the kernels above.
struct CovarGeom {
  float m[3], cv[6], q0[3], q1[3];
};

// Gaussian g in camera `cam_id`: the forward of the pair (false = culled); m and cv are loaded on the way
template <int CM>
__device__ __forceinline__ bool packed_geom_covar(const float *__restrict__ means, const float *__restrict__ covars,
                                                  const float *__restrict__ viewmats, const float *__restrict__ Ks,
                                                  int cam_id, int g, int width, int height, float near_plane,
                                                  float far_plane, float eps2d, Cam &cam, CovarGeom &cg, Fwd &f) {
  cam = load_cam(viewmats + 16 * (size_t)cam_id, Ks + 9 * (size_t)cam_id);
#pragma unroll
  for (int k = 0; k < 3; ++k) cg.m[k] = means[3 * (size_t)g + k];
#pragma unroll
  for (int k = 0; k < 6; ++k) cg.cv[k] = covars[6 * (size_t)g + k];
  float cc[6];
  return forward_geom_covar<CM>(cam, cg.m, cg.cv, width, height, near_plane, far_plane, eps2d, f, cc, cg.q0, cg.q1);
}

// radius after every cull (0 = not kept) of this thread's Gaussian in camera blockIdx.y
template <int CM>
__device__ __forceinline__ int packed_project_covar(const float *__restrict__ means, const float *__restrict__ covars,
                                                    const float *__restrict__ viewmats, const float *__restrict__ Ks,
                                                    int N, int width, int height, float near_plane, float far_plane,
                                                    float eps2d, float radius_clip, int g, Fwd &f) {
  if (g >= N) return 0;
  Cam cam;
  CovarGeom cg;
  if (!packed_geom_covar<CM>(means, covars, viewmats, Ks, blockIdx.y, g, width, height, near_plane, far_plane, eps2d, cam,
                             cg, f))
    return 0;
  return radius_of(f, width, height, radius_clip);
}

template <int CM>
__global__ void __launch_bounds__(kPk)
packed_count_covars_kernel(const float *__restrict__ means, const float *__restrict__ covars,
                           const float *__restrict__ viewmats, const float *__restrict__ Ks, int N, int width,
                           int height, float near_plane, float far_plane, float eps2d, float radius_clip,
                           int *__restrict__ block_counts) {
  __shared__ int s_wave[kPk / 64];
  const int g = blockIdx.x * kPk + threadIdx.x;
  Fwd f;
  const int radius = packed_project_covar<CM>(means, covars, viewmats, Ks, N, width, height, near_plane, far_plane, eps2d,
                                              radius_clip, g, f);
  const unsigned long long vote = __ballot(radius > 0);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(vote);
  __syncthreads();
  if (threadIdx.x == 0)
    block_counts[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// (forward_geom_covar does not fill f.o: the record's opacity comes straight from opacities[g])
template <bool LDS_COUNT, int CM>
__global__ void __launch_bounds__(kPk)
packed_write_covars_kernel(const float *__restrict__ means, const float *__restrict__ covars,
                           const float *__restrict__ opacities, const float *__restrict__ viewmats,
                           const float *__restrict__ Ks, int N, int width, int height, float near_plane,
                           float far_plane, float eps2d, float radius_clip, uint32_t flags,
                           const int *__restrict__ block_base, long long nnz, float4 *__restrict__ splat,
                           int *__restrict__ radii, float *__restrict__ means2d, float *__restrict__ depths,
                           float *__restrict__ conics, float *__restrict__ comps, int *__restrict__ tiles_per_gauss,
                           long long *__restrict__ camera_ids, long long *__restrict__ gaussian_ids,
                           int *__restrict__ tile_counts) {
  extern __shared__ __attribute__((aligned(16))) int s_hist[];
  __shared__ int s_wave[kPk / 64];
  const int tw = (width + kTile - 1) / kTile, th = (height + kTile - 1) / kTile, T = tw * th;
  tile_counts += (size_t)blockIdx.y * T;
  if (LDS_COUNT) {
    for (int t = threadIdx.x; t < T; t += kPk) s_hist[t] = 0;
  }
  const int g = blockIdx.x * kPk + threadIdx.x;
  Fwd f;
  const int radius = packed_project_covar<CM>(means, covars, viewmats, Ks, N, width, height, near_plane, far_plane, eps2d,
                                              radius_clip, g, f);
  const bool keep = radius > 0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long vote = __ballot(keep);
  if (lane == 0) s_wave[wv] = __popcll(vote);
  __syncthreads();  // (also: the histogram is zero)
  if (!keep) {
    if (!LDS_COUNT) return;
  } else {
    long long p = block_base[(size_t)blockIdx.y * gridDim.x + blockIdx.x] + __popcll(vote & ((1ull << lane) - 1ull));
    for (int w = 0; w < wv; ++w) p += s_wave[w];
    if (p >= 0 && p < nnz) {  // (always: nnz is the sum the bases were scanned from -- a guard against a caller's stale scratch)
      const bool aa = flags & EG_FLAG_ANTIALIASED;
      const float o = opacities[g];
      splat[2 * p] = make_float4(f.u, f.v, f.a, f.b);
      splat[2 * p + 1] = make_float4(f.c, aa ? o * f.comp : o, f.z, __int_as_float(radius));
      radii[p] = radius;
      means2d[2 * p] = f.u; means2d[2 * p + 1] = f.v;
      depths[p] = f.z;
      conics[3 * p] = f.a; conics[3 * p + 1] = f.b; conics[3 * p + 2] = f.c;
      comps[p] = f.comp;
      camera_ids[p] = blockIdx.y;
      gaussian_ids[p] = g;
      int x0, y0, x1, y1;
      tile_box(f.u, f.v, radius, tw, th, x0, y0, x1, y1);
      tiles_per_gauss[p] = (y1 - y0) * (x1 - x0);
      for (int ty = y0; ty < y1; ++ty)
        for (int tx = x0; tx < x1; ++tx) atomicAdd(LDS_COUNT ? &s_hist[ty * tw + tx] : &tile_counts[ty * tw + tx], 1);
    }
  }
  if (LDS_COUNT) {
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += kPk) {
      const int c = s_hist[t];
      if (c) atomicAdd(&tile_counts[t], c);
    }
  }
}

// one pair's share of v_means [3] and v_covars [6] (csrc/covar_dev.h); zeros should the recomputed forward cull it
template <int CM>
__device__ __forceinline__ void packed_pair_vjp_covar(const float *__restrict__ means, const float *__restrict__ covars,
                                                      const float *__restrict__ viewmats, const float *__restrict__ Ks,
                                                      int cam_id, int g, long long p, int width, int height, float eps2d,
                                                      uint32_t flags, const float4 *__restrict__ g2d,
                                                      const float *__restrict__ v_comps,
                                                      const float *__restrict__ v_depths, float (&gm)[3], float (&gc)[6]) {
  Cam cam;
  CovarGeom cg;
  Fwd f;
#pragma unroll
  for (int k = 0; k < 3; ++k) gm[k] = 0.f;
#pragma unroll
  for (int k = 0; k < 6; ++k) gc[k] = 0.f;
  // near / far already passed in the forward (the pair exists), so pass open limits
  if (!packed_geom_covar<CM>(means, covars, viewmats, Ks, cam_id, g, width, height, -3.0e38f, 3.0e38f, eps2d, cam, cg, f))
    return;
  const CovarCot ct = load_covar_cot(g2d, v_comps, v_depths, p, flags & EG_FLAG_ANTIALIASED);
  covar_pair_vjp<false, CM>(cam, cg.m, cg.cv, f, cg.q0, cg.q1, eps2d, ct, gm, gc);
}

template <int CM>
__global__ void __launch_bounds__(256)
packed_bwd_dense_covars_kernel(const float *__restrict__ means, const float *__restrict__ covars,
                               const float *__restrict__ viewmats, const float *__restrict__ Ks, int N, int C, int width,
                               int height, float eps2d, uint32_t flags, const long long *__restrict__ indptr,
                               long long nnz, const long long *__restrict__ gaussian_ids,
                               const float4 *__restrict__ g2d, const float *__restrict__ v_comps,
                               const float *__restrict__ v_depths, float *__restrict__ v_means,
                               float *__restrict__ v_covars) {
#pragma clang fp contract(off)  // (the same bits whatever the compiler makes of the camera loop)
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= N) return;
  float am[3] = {0.f, 0.f, 0.f}, ac[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < C; ++c) {
    const long long end = min(indptr[c + 1], nnz);  // (indptr is the scan's: a guard against a caller's stale array)
    long long lo = max(0ll, indptr[c]);
    long long hi = end;
    while (lo < hi) {  // first position whose id is >= g
      const long long mid = lo + ((hi - lo) >> 1);
      if (gaussian_ids[mid] < g) lo = mid + 1; else hi = mid;
    }
    if (lo >= end || gaussian_ids[lo] != g) continue;
    float gm[3], gc[6];
    packed_pair_vjp_covar<CM>(means, covars, viewmats, Ks, c, g, lo, width, height, eps2d, flags, g2d, v_comps, v_depths,
                              gm, gc);
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

template <int CM>
__global__ void __launch_bounds__(256)
packed_bwd_sparse_covars_kernel(const float *__restrict__ means, const float *__restrict__ covars,
                                const float *__restrict__ viewmats, const float *__restrict__ Ks, int N, int C,
                                int width, int height, float eps2d, uint32_t flags, long long nnz,
                                const long long *__restrict__ camera_ids, const long long *__restrict__ gaussian_ids,
                                const float4 *__restrict__ g2d, const float *__restrict__ v_comps,
                                const float *__restrict__ v_depths, float *__restrict__ v_means,
                                float *__restrict__ v_covars) {
  const long long p = blockIdx.x * 256ll + threadIdx.x;
  if (p >= nnz) return;
  const long long c = camera_ids[p], g = gaussian_ids[p];
  float gm[3] = {0.f, 0.f, 0.f}, gc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c >= 0 && c < C && g >= 0 && g < N)  // (ids written by packed_write_covars_kernel: a guard against a caller's stale arrays)
    packed_pair_vjp_covar<CM>(means, covars, viewmats, Ks, (int)c, (int)g, p, width, height, eps2d, flags, g2d, v_comps,
                              v_depths, gm, gc);
#pragma unroll
  for (int k = 0; k < 3; ++k) v_means[3 * p + k] = gm[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) v_covars[6 * p + k] = gc[k];
}

}  // namespace eg

using namespace eg;

#define EG_PACKED_SIZES(N, C, width, height)                                                        \
  EG_REQUIRE(N >= 0 && C >= 1 && C <= 65535 && width > 0 && height > 0, "bad sizes")

extern "C" int eg_packed_count(const float *means, const float *quats, const float *scales, const float *opacities,
                               const float *viewmats, const float *Ks, int32_t N, int32_t C, int32_t width,
                               int32_t height, float near_plane, float far_plane, float eps2d, float radius_clip,
                               uint32_t flags, int32_t *block_base, int64_t *indptr, eg_stream_t stream) {
  EG_PACKED_SIZES(N, C, width, height);
  EG_REQUIRE(viewmats && Ks && indptr, "null pointer");
  EG_REQUIRE(N == 0 || (means && quats && scales && opacities && block_base), "null pointer");
  hipStream_t s = as_stream(stream);
  const int nb = cdiv(N, kPk);
#define EG_PACKED_COUNT(CM_)                                                                                       \
  packed_count_kernel<CM_><<<dim3(nb, C), kPk, 0, s>>>(means, quats, scales, opacities, viewmats, Ks, N, width, height, \
                                                       near_plane, far_plane, eps2d, radius_clip, flags, block_base)
  if (N > 0) {
    if (flags & EG_FLAG_ORTHO) EG_PACKED_COUNT(kOrtho); else EG_PACKED_COUNT(kPinhole);
  }
#undef EG_PACKED_COUNT
  packed_scan_kernel<<<1, 256, 0, s>>>(block_base, nb, C, (long long *)indptr);
  return check_launch("packed_count");
}

extern "C" int eg_packed_write(const float *means, const float *quats, const float *scales, const float *opacities,
                               const float *viewmats, const float *Ks, int32_t N, int32_t C, int32_t width,
                               int32_t height, float near_plane, float far_plane, float eps2d, float radius_clip,
                               uint32_t flags, const int32_t *block_base, int64_t nnz, float *splat, int32_t *radii,
                               float *means2d, float *depths, float *conics, float *compensations,
                               int32_t *tiles_per_gauss, int64_t *camera_ids, int64_t *gaussian_ids,
                               int32_t *tile_counts, eg_stream_t stream) {
  EG_PACKED_SIZES(N, C, width, height);
  EG_REQUIRE(nnz >= 0 && nnz <= (int64_t)N * C && nnz < (1ll << 31), "bad nnz");
  if (nnz == 0) return EG_OK;
  EG_REQUIRE(means && quats && scales && opacities && viewmats && Ks && block_base && splat && radii && means2d &&
                 depths && conics && compensations && tiles_per_gauss && camera_ids && gaussian_ids && tile_counts,
             "null pointer");
  hipStream_t s = as_stream(stream);
  const int T = cdiv(width, kTile) * cdiv(height, kTile);
#define EG_PACKED_WRITE(LDS, CM_, SMEM)                                                                              \
  packed_write_kernel<LDS, CM_><<<dim3(cdiv(N, kPk), C), kPk, SMEM, s>>>(                                            \
      means, quats, scales, opacities, viewmats, Ks, N, width, height, near_plane, far_plane, eps2d, radius_clip,    \
      flags, block_base, (long long)nnz, (float4 *)splat, radii, means2d, depths, conics, compensations,             \
      tiles_per_gauss, (long long *)camera_ids, (long long *)gaussian_ids, tile_counts)
  if (flags & EG_FLAG_ORTHO) {
    if (T <= 16384) EG_PACKED_WRITE(true, kOrtho, sizeof(int) * T); else EG_PACKED_WRITE(false, kOrtho, 0);
  } else {
    if (T <= 16384) EG_PACKED_WRITE(true, kPinhole, sizeof(int) * T); else EG_PACKED_WRITE(false, kPinhole, 0);
  }
#undef EG_PACKED_WRITE
  return check_launch("packed_write");
}

// Binning of every camera's range of the packed list: indptr_host [C + 1], offsets [C, T + 1] (eg_tile_offsets_cams),
// tile_counts [C, T] (returned to zero), M_host [C]; keys / flatten_ids / isect_ids hold sum(M_host) entries, camera
// c's at sum(M_host[:c]).  flatten_ids come out as indices into the whole packed list, isect_ids (NULL ok) with the
// camera in the bits above the tile's.
extern "C" int eg_packed_bin(const float *means2d, const int32_t *radii, const float *depths,
                             const int64_t *indptr_host, int32_t C, int32_t width, int32_t height,
                             const int32_t *offsets, int32_t *tile_counts, const int64_t *M_host, uint64_t *keys,
                             int32_t *flatten_ids, int64_t *isect_ids, const int32_t *max_tile_host,
                             eg_stream_t stream) {
  EG_REQUIRE(C >= 1 && width > 0 && height > 0, "bad sizes");
  EG_REQUIRE(indptr_host && offsets && tile_counts && M_host, "null pointer");
  const int T = cdiv(width, kTile) * cdiv(height, kTile);
  int tile_bits = 0;
  while ((1 << tile_bits) <= T) ++tile_bits;  // floor(log2(T)) + 1
  EG_REQUIRE(indptr_host[0] == 0, "indptr must start at 0");
  for (int c = 0; c < C; ++c) {  // (everything is checked before the first launch)
    const int64_t n = indptr_host[c + 1] - indptr_host[c], M = M_host[c];
    EG_REQUIRE(n >= 0 && indptr_host[c + 1] < (1ll << 31) && M >= 0, "bad sizes");
    EG_REQUIRE(M == 0 || (n > 0 && means2d && radii && depths && keys && flatten_ids), "null pointer");
  }
  int64_t m_base = 0;
  for (int c = 0; c < C; ++c) {
    const int64_t b = indptr_host[c], n = indptr_host[c + 1] - b, M = M_host[c];
    if (M > 0) {
      const int32_t *offs = offsets + (size_t)(T + 1) * c;
      int rc = eg_tile_emit(means2d + 2 * b, radii + b, depths + b, nullptr, 0, (int32_t)n, width, height, offs,
                            tile_counts + (size_t)T * c, M, keys + m_base, nullptr, stream);
      if (rc) return rc;
      int64_t *ids = isect_ids ? isect_ids + m_base : nullptr;
      rc = eg_sort_pairs(keys + m_base, offs, T, M, flatten_ids + m_base, ids, max_tile_host ? max_tile_host[c] : 0, stream);
      if (rc) return rc;
      if (b > 0 || (ids && c > 0)) {
        packed_rebase_kernel<<<cdiv(M, 256), 256, 0, as_stream(stream)>>>(
            flatten_ids + m_base, (long long *)ids, (long long)M, (int)b, (long long)c << (32 + tile_bits));
        rc = check_launch("packed_bin");
        if (rc) return rc;
      }
    }
    m_base += M;
  }
  return EG_OK;
}

// v_means [N,3], v_quats [N,4], v_scales [N,3]: the sum over the cameras in camera order, every row written
extern "C" int eg_packed_bwd(const float *means, const float *quats, const float *scales, const float *opacities,
                             const float *viewmats, const float *Ks, int32_t N, int32_t C, int32_t width,
                             int32_t height, float eps2d, uint32_t flags, const int64_t *indptr, int64_t nnz,
                             const int64_t *gaussian_ids, const float *g2d, const float *v_comps,
                             const float *v_depths, float *v_means, float *v_quats, float *v_scales,
                             eg_stream_t stream) {
  EG_PACKED_SIZES(N, C, width, height);
  EG_REQUIRE(nnz >= 0 && nnz <= (int64_t)N * C, "bad nnz");
  if (N == 0) return EG_OK;
  EG_REQUIRE(means && quats && scales && opacities && viewmats && Ks && indptr && v_means && v_quats && v_scales,
             "null pointer");
  EG_REQUIRE(nnz == 0 || (gaussian_ids && g2d && v_comps), "null pointer");
#define EG_PACKED_BWD(CM_)                                                                                           \
  packed_bwd_dense_kernel<CM_><<<cdiv(N, 256), 256, 0, as_stream(stream)>>>(                                         \
      means, quats, scales, opacities, viewmats, Ks, N, C, width, height, eps2d, flags, (const long long *)indptr,   \
      (long long)nnz, (const long long *)gaussian_ids, (const float4 *)g2d, v_comps, v_depths, v_means, v_quats, v_scales)
  if (flags & EG_FLAG_ORTHO) EG_PACKED_BWD(kOrtho); else EG_PACKED_BWD(kPinhole);
#undef EG_PACKED_BWD
  return check_launch("packed_bwd");
}

// the values of the sparse gradients: v_means [nnz,3], v_quats [nnz,4], v_scales [nnz,3], one row per pair
extern "C" int eg_packed_bwd_sparse(const float *means, const float *quats, const float *scales,
                                    const float *opacities, const float *viewmats, const float *Ks, int32_t N,
                                    int32_t C, int32_t width, int32_t height, float eps2d, uint32_t flags, int64_t nnz,
                                    const int64_t *camera_ids, const int64_t *gaussian_ids, const float *g2d,
                                    const float *v_comps, const float *v_depths, float *v_means, float *v_quats,
                                    float *v_scales, eg_stream_t stream) {
  EG_PACKED_SIZES(N, C, width, height);
  EG_REQUIRE(nnz >= 0 && nnz <= (int64_t)N * C && nnz < (1ll << 31), "bad nnz");
  if (nnz == 0) return EG_OK;
  EG_REQUIRE(means && quats && scales && opacities && viewmats && Ks && camera_ids && gaussian_ids && g2d && v_comps &&
                 v_means && v_quats && v_scales,
             "null pointer");
#define EG_PACKED_BWD_SPARSE(CM_)                                                                                    \
  packed_bwd_sparse_kernel<CM_><<<cdiv(nnz, 256), 256, 0, as_stream(stream)>>>(                                      \
      means, quats, scales, opacities, viewmats, Ks, N, C, width, height, eps2d, flags, (long long)nnz,              \
      (const long long *)camera_ids, (const long long *)gaussian_ids, (const float4 *)g2d, v_comps, v_depths, v_means, \
      v_quats, v_scales)
  if (flags & EG_FLAG_ORTHO) EG_PACKED_BWD_SPARSE(kOrtho); else EG_PACKED_BWD_SPARSE(kPinhole);
#undef EG_PACKED_BWD_SPARSE
  return check_launch("packed_bwd_sparse");
}

// ---- the covariance form: covars [N, 6] (upper triangle) in place of quats + scales; scan, eg_packed_bin and the rebase
// are the ones above
extern "C" int eg_packed_count_covars(const float *means, const float *covars, const float *viewmats, const float *Ks,
                                      int32_t N, int32_t C, int32_t width, int32_t height, float near_plane,
                                      float far_plane, float eps2d, float radius_clip, uint32_t flags,
                                      int32_t *block_base, int64_t *indptr, eg_stream_t stream) {
  EG_PACKED_SIZES(N, C, width, height);
  EG_REQUIRE(viewmats && Ks && indptr, "null pointer");
  EG_REQUIRE(N == 0 || (means && covars && block_base), "null pointer");
  hipStream_t s = as_stream(stream);
  const int nb = cdiv(N, kPk);
#define EG_PACKED_COUNT(CM_)                                                                                       \
  packed_count_covars_kernel<CM_><<<dim3(nb, C), kPk, 0, s>>>(means, covars, viewmats, Ks, N, width, height, near_plane, \
                                                              far_plane, eps2d, radius_clip, block_base)
  if (N > 0) {
    if (flags & EG_FLAG_ORTHO) EG_PACKED_COUNT(kOrtho); else EG_PACKED_COUNT(kPinhole);
  }
#undef EG_PACKED_COUNT
  packed_scan_kernel<<<1, 256, 0, s>>>(block_base, nb, C, (long long *)indptr);
  return check_launch("packed_count_covars");
}

extern "C" int eg_packed_write_covars(const float *means, const float *covars, const float *opacities,
                                      const float *viewmats, const float *Ks, int32_t N, int32_t C, int32_t width,
                                      int32_t height, float near_plane, float far_plane, float eps2d, float radius_clip,
                                      uint32_t flags, const int32_t *block_base, int64_t nnz, float *splat,
                                      int32_t *radii, float *means2d, float *depths, float *conics,
                                      float *compensations, int32_t *tiles_per_gauss, int64_t *camera_ids,
                                      int64_t *gaussian_ids, int32_t *tile_counts, eg_stream_t stream) {
  EG_PACKED_SIZES(N, C, width, height);
  EG_REQUIRE(nnz >= 0 && nnz <= (int64_t)N * C && nnz < (1ll << 31), "bad nnz");
  if (nnz == 0) return EG_OK;
  EG_REQUIRE(means && covars && opacities && viewmats && Ks && block_base && splat && radii && means2d && depths &&
                 conics && compensations && tiles_per_gauss && camera_ids && gaussian_ids && tile_counts,
             "null pointer");
  hipStream_t s = as_stream(stream);
  const int T = cdiv(width, kTile) * cdiv(height, kTile);
#define EG_PACKED_WRITE(LDS, CM_, SMEM)                                                                              \
  packed_write_covars_kernel<LDS, CM_><<<dim3(cdiv(N, kPk), C), kPk, SMEM, s>>>(                                     \
      means, covars, opacities, viewmats, Ks, N, width, height, near_plane, far_plane, eps2d, radius_clip, flags,    \
      block_base, (long long)nnz, (float4 *)splat, radii, means2d, depths, conics, compensations, tiles_per_gauss,   \
      (long long *)camera_ids, (long long *)gaussian_ids, tile_counts)
  if (flags & EG_FLAG_ORTHO) {
    if (T <= 16384) EG_PACKED_WRITE(true, kOrtho, sizeof(int) * T); else EG_PACKED_WRITE(false, kOrtho, 0);
  } else {
    if (T <= 16384) EG_PACKED_WRITE(true, kPinhole, sizeof(int) * T); else EG_PACKED_WRITE(false, kPinhole, 0);
  }
#undef EG_PACKED_WRITE
  return check_launch("packed_write_covars");
}

// v_means [N,3], v_covars [N,6]: the sum over the cameras in camera order, every row written
extern "C" int eg_packed_bwd_covars(const float *means, const float *covars, const float *viewmats, const float *Ks,
                                    int32_t N, int32_t C, int32_t width, int32_t height, float eps2d, uint32_t flags,
                                    const int64_t *indptr, int64_t nnz, const int64_t *gaussian_ids, const float *g2d,
                                    const float *v_comps, const float *v_depths, float *v_means, float *v_covars,
                                    eg_stream_t stream) {
  EG_PACKED_SIZES(N, C, width, height);
  EG_REQUIRE(nnz >= 0 && nnz <= (int64_t)N * C, "bad nnz");
  if (N == 0) return EG_OK;
  EG_REQUIRE(means && covars && viewmats && Ks && indptr && v_means && v_covars, "null pointer");
  EG_REQUIRE(nnz == 0 || (gaussian_ids && g2d && v_comps), "null pointer");
#define EG_PACKED_BWD(CM_)                                                                                           \
  packed_bwd_dense_covars_kernel<CM_><<<cdiv(N, 256), 256, 0, as_stream(stream)>>>(                                  \
      means, covars, viewmats, Ks, N, C, width, height, eps2d, flags, (const long long *)indptr, (long long)nnz,     \
      (const long long *)gaussian_ids, (const float4 *)g2d, v_comps, v_depths, v_means, v_covars)
  if (flags & EG_FLAG_ORTHO) EG_PACKED_BWD(kOrtho); else EG_PACKED_BWD(kPinhole);
#undef EG_PACKED_BWD
  return check_launch("packed_bwd_covars");
}

// the values of the sparse gradients: v_means [nnz,3], v_covars [nnz,6], one row per pair
extern "C" int eg_packed_bwd_sparse_covars(const float *means, const float *covars, const float *viewmats,
                                           const float *Ks, int32_t N, int32_t C, int32_t width, int32_t height,
                                           float eps2d, uint32_t flags, int64_t nnz, const int64_t *camera_ids,
                                           const int64_t *gaussian_ids, const float *g2d, const float *v_comps,
                                           const float *v_depths, float *v_means, float *v_covars,
                                           eg_stream_t stream) {
  EG_PACKED_SIZES(N, C, width, height);
  EG_REQUIRE(nnz >= 0 && nnz <= (int64_t)N * C && nnz < (1ll << 31), "bad nnz");
  if (nnz == 0) return EG_OK;
  EG_REQUIRE(means && covars && viewmats && Ks && camera_ids && gaussian_ids && g2d && v_comps && v_means && v_covars,
             "null pointer");
#define EG_PACKED_BWD_SPARSE(CM_)                                                                                    \
  packed_bwd_sparse_covars_kernel<CM_><<<cdiv(nnz, 256), 256, 0, as_stream(stream)>>>(                               \
      means, covars, viewmats, Ks, N, C, width, height, eps2d, flags, (long long)nnz, (const long long *)camera_ids, \
      (const long long *)gaussian_ids, (const float4 *)g2d, v_comps, v_depths, v_means, v_covars)
  if (flags & EG_FLAG_ORTHO) EG_PACKED_BWD_SPARSE(kOrtho); else EG_PACKED_BWD_SPARSE(kPinhole);
#undef EG_PACKED_BWD_SPARSE
  return check_launch("packed_bwd_sparse_covars");
}
