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
//   bin     camera c's range is a single-camera problem: the general path's per-camera binning step (bin_camera,
//           binning.hip: emission, eg_sort_pairs, rebase) through base pointers, with indptr[c] as the id base -- the
//           sorted ids index the whole packed list -- and the camera in the isect ids.
//   bwd     dense gradients: one thread per Gaussian walks the cameras 0 .. C-1 (eg_project_bwd_cams's order), finds
//           its pair by binary search in the camera's ascending ids, sums in registers, writes every row once (zeros
//           where nobody sees it).  No atomics, no zero-fill: bit-identical from run to run.
//           sparse gradients: one thread per pair, no reduction.
//
// Scratch: 4 bytes per 256 pairs (the workgroup counts).  Nothing of size C * N is allocated.
//
// Count, write and the two backwards are templates over the form the Gaussian's shape arrives in: QuatScaleForm
// (csrc/project_dev.h) behind eg_packed_*, CovarForm (csrc/covar_dev.h; gsplat `rasterization(covars=[N, 3, 3])`, the
// upper triangle covars [N, 6]) behind eg_packed_*_covars.  A form brings its inputs, the forward of a pair, the
// record's opacity, its gradient row and the pair's reverse sweep; everything else -- grids, ranking, histogram, guards,
// the order of the sums -- is written once.  The covariance form's keep decision is forward_geom_covar + radius_of with
// the arguments of project_covars_fwd_kernel (csrc/functional.hip): its kept set is the set radii > 0 of
// eg_project_covars_fwd_cams_flags, every kept value bit for bit.
#include "common.h"
#include "covar_dev.h"
#include "project_dev.h"

namespace eg {

constexpr int kPk = 256;  // threads (= Gaussians) per workgroup of the count and write passes

// the cameras and the projection's scalars, as every kernel here takes them (the backwards read no cull limit)
struct PackedView {
  const float *viewmats, *Ks;
  int N, C, width, height;
  float near_plane, far_plane, eps2d, radius_clip;
  uint32_t flags;
};

// this thread's Gaussian in camera blockIdx.y: radius after every cull (0 = not kept).  CM: the camera model
// (csrc/project_dev.h) of every kernel here, kOrtho with EG_FLAG_ORTHO.
template <class Form, int CM>
__device__ __forceinline__ int packed_project(Form &form, const PackedView &v, int g, Fwd &f) {
  if (g >= v.N) return 0;
  const Cam cam = load_cam(v.viewmats + 16 * (size_t)blockIdx.y, v.Ks + 9 * (size_t)blockIdx.y);
  if (!form.template forward<CM>(cam, g, v.width, v.height, v.near_plane, v.far_plane, v.eps2d, v.flags, f)) return 0;
  return radius_of(f, v.width, v.height, v.radius_clip);
}

template <class Form, int CM>
__global__ void __launch_bounds__(kPk)
packed_count_kernel(Form form, const PackedView v, int *__restrict__ block_counts) {
  __shared__ int s_wave[kPk / 64];
  const int g = blockIdx.x * kPk + threadIdx.x;
  Fwd f;
  const int radius = packed_project<Form, CM>(form, v, g, f);
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

// the outputs of the write pass, one row per kept pair (tile_counts: [C, T])
struct PackedOut {
  float4 *splat;
  int *radii;
  float *means2d, *depths, *conics, *comps;
  int *tiles_per_gauss;
  long long *camera_ids, *gaussian_ids;
  int *tile_counts;
};

template <class Form, bool LDS_COUNT, int CM>
__global__ void __launch_bounds__(kPk)
packed_write_kernel(Form form, const PackedView v, const int *__restrict__ block_base, long long nnz,
                    const PackedOut o) {
  extern __shared__ __attribute__((aligned(16))) int s_hist[];
  __shared__ int s_wave[kPk / 64];
  const int tw = (v.width + kTile - 1) / kTile, th = (v.height + kTile - 1) / kTile, T = tw * th;
  int *tile_counts = o.tile_counts + (size_t)blockIdx.y * T;
  if (LDS_COUNT) {
    for (int t = threadIdx.x; t < T; t += kPk) s_hist[t] = 0;
  }
  const int g = blockIdx.x * kPk + threadIdx.x;
  Fwd f;
  const int radius = packed_project<Form, CM>(form, v, g, f);
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
      const bool aa = v.flags & EG_FLAG_ANTIALIASED;
      const float op = form.opacity(f, g);
      o.splat[2 * p] = make_float4(f.u, f.v, f.a, f.b);
      o.splat[2 * p + 1] = make_float4(f.c, aa ? op * f.comp : op, f.z, __int_as_float(radius));
      o.radii[p] = radius;
      o.means2d[2 * p] = f.u; o.means2d[2 * p + 1] = f.v;
      o.depths[p] = f.z;
      o.conics[3 * p] = f.a; o.conics[3 * p + 1] = f.b; o.conics[3 * p + 2] = f.c;
      o.comps[p] = f.comp;
      o.camera_ids[p] = blockIdx.y;
      o.gaussian_ids[p] = g;
      int x0, y0, x1, y1;
      tile_box(f.u, f.v, radius, tw, th, x0, y0, x1, y1);
      o.tiles_per_gauss[p] = (y1 - y0) * (x1 - x0);
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

// the cotangents of the pairs: the [nnz, 8] record of the compositing backwards, v_comps [nnz], v_depths [nnz] (NULL ok)
struct PackedCot {
  const float4 *g2d;
  const float *v_comps, *v_depths;
};

// pair p = (cam_id, g): its share of row g's gradient (zero on entry)
template <class Form, int CM>
__device__ __forceinline__ void packed_pair_vjp(Form &form, const PackedView &v, int cam_id, int g, long long p,
                                                const PackedCot &ct, typename Form::Grad &gr) {
  const Cam cam = load_cam(v.viewmats + 16 * (size_t)cam_id, v.Ks + 9 * (size_t)cam_id);
  form.template pair_vjp<false, CM>(cam, g, p, v.width, v.height, v.eps2d, v.flags, ct.g2d, ct.v_comps, ct.v_depths, gr);
}

template <class Form, int CM>
__global__ void __launch_bounds__(256)
packed_bwd_dense_kernel(Form form, const PackedView v, const long long *__restrict__ indptr, long long nnz,
                        const long long *__restrict__ gaussian_ids, const PackedCot ct,
                        const typename Form::Out out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= v.N) return;
  typename Form::Grad acc;
  acc.zero();
  for (int c = 0; c < v.C; ++c) {
    const long long end = min(indptr[c + 1], nnz);  // (indptr is the scan's: a guard against a caller's stale array)
    long long lo = max(0ll, indptr[c]);
    long long hi = end;
    while (lo < hi) {  // first position whose id is >= g
      const long long mid = lo + ((hi - lo) >> 1);
      if (gaussian_ids[mid] < g) lo = mid + 1; else hi = mid;
    }
    if (lo >= end || gaussian_ids[lo] != g) continue;
    typename Form::Grad gr;
    gr.zero();
    packed_pair_vjp<Form, CM>(form, v, c, g, lo, ct, gr);
    acc += gr;
  }
  acc.store(out, g);
}

template <class Form, int CM>
__global__ void __launch_bounds__(256)
packed_bwd_sparse_kernel(Form form, const PackedView v, long long nnz, const long long *__restrict__ camera_ids,
                         const long long *__restrict__ gaussian_ids, const PackedCot ct,
                         const typename Form::Out out) {
  const long long p = blockIdx.x * 256ll + threadIdx.x;
  if (p >= nnz) return;
  const long long c = camera_ids[p], g = gaussian_ids[p];
  typename Form::Grad gr;
  gr.zero();
  if (c >= 0 && c < v.C && g >= 0 && g < v.N)  // (ids written by packed_write_kernel: a guard against a caller's stale arrays)
    packed_pair_vjp<Form, CM>(form, v, (int)c, (int)g, p, ct, gr);
  gr.store(out, p);
}

}  // namespace eg

using namespace eg;

// ---- one host launcher per pass: it owns the camera-model (and, write, the histogram) dispatch; the entries below
// check their own arguments and name themselves to check_launch
template <class Form>
static void launch_count(const Form &form, const PackedView &v, int32_t *block_base, int64_t *indptr, hipStream_t s) {
  const int nb = cdiv(v.N, kPk);
  if (v.N > 0)
    with_cam_model(v.flags, [&](auto cm) {
      packed_count_kernel<Form, decltype(cm)::value><<<dim3(nb, v.C), kPk, 0, s>>>(form, v, block_base);
    });
  packed_scan_kernel<<<1, 256, 0, s>>>(block_base, nb, v.C, (long long *)indptr);
}

template <class Form>
static void launch_write(const Form &form, const PackedView &v, const int32_t *block_base, int64_t nnz,
                         const PackedOut &o, hipStream_t s) {
  const int T = cdiv(v.width, kTile) * cdiv(v.height, kTile);
  const dim3 grid(cdiv(v.N, kPk), v.C);
  with_cam_model(v.flags, [&](auto cm) {
    constexpr int CM = decltype(cm)::value;
    if (T <= 16384)
      packed_write_kernel<Form, true, CM><<<grid, kPk, sizeof(int) * T, s>>>(form, v, block_base, (long long)nnz, o);
    else
      packed_write_kernel<Form, false, CM><<<grid, kPk, 0, s>>>(form, v, block_base, (long long)nnz, o);
  });
}

template <class Form>
static void launch_bwd_dense(const Form &form, const PackedView &v, const int64_t *indptr, int64_t nnz,
                             const int64_t *gaussian_ids, const PackedCot &ct, const typename Form::Out &out,
                             hipStream_t s) {
  with_cam_model(v.flags, [&](auto cm) {
    packed_bwd_dense_kernel<Form, decltype(cm)::value><<<cdiv(v.N, 256), 256, 0, s>>>(
        form, v, (const long long *)indptr, (long long)nnz, (const long long *)gaussian_ids, ct, out);
  });
}

template <class Form>
static void launch_bwd_sparse(const Form &form, const PackedView &v, int64_t nnz, const int64_t *camera_ids,
                              const int64_t *gaussian_ids, const PackedCot &ct, const typename Form::Out &out,
                              hipStream_t s) {
  with_cam_model(v.flags, [&](auto cm) {
    packed_bwd_sparse_kernel<Form, decltype(cm)::value><<<cdiv(nnz, 256), 256, 0, s>>>(
        form, v, (long long)nnz, (const long long *)camera_ids, (const long long *)gaussian_ids, ct, out);
  });
}

#define EG_PACKED_SIZES(N, C, width, height)                                                        \
  EG_REQUIRE(N >= 0 && C >= 1 && C <= 65535 && width > 0 && height > 0, "bad sizes")

extern "C" int eg_packed_count(const float *means, const float *quats, const float *scales, const float *opacities,
                               const float *viewmats, const float *Ks, int32_t N, int32_t C, int32_t width,
                               int32_t height, float near_plane, float far_plane, float eps2d, float radius_clip,
                               uint32_t flags, int32_t *block_base, int64_t *indptr, eg_stream_t stream) {
  EG_PACKED_SIZES(N, C, width, height);
  EG_REQUIRE(viewmats && Ks && indptr, "null pointer");
  EG_REQUIRE(N == 0 || (means && quats && scales && opacities && block_base), "null pointer");
  launch_count(QuatScaleForm{means, quats, scales, opacities},
               PackedView{viewmats, Ks, N, C, width, height, near_plane, far_plane, eps2d, radius_clip, flags},
               block_base, indptr, as_stream(stream));
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
  launch_write(QuatScaleForm{means, quats, scales, opacities},
               PackedView{viewmats, Ks, N, C, width, height, near_plane, far_plane, eps2d, radius_clip, flags},
               block_base, nnz,
               PackedOut{(float4 *)splat, radii, means2d, depths, conics, compensations, tiles_per_gauss,
                         (long long *)camera_ids, (long long *)gaussian_ids, tile_counts},
               as_stream(stream));
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
  const int tw = cdiv(width, kTile), th = cdiv(height, kTile), T = tw * th;
  const int bits = tile_bits(T);
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
      const int rc = bin_camera("packed_bin", means2d + 2 * b, radii + b, depths + b, (int)n, kTile, tw, th,
                                offsets + (size_t)(T + 1) * c, tile_counts + (size_t)T * c, M, keys + m_base,
                                flatten_ids + m_base, isect_ids ? isect_ids + m_base : nullptr,
                                max_tile_host ? max_tile_host[c] : 0, (int)b, (int64_t)c << (32 + bits), stream);
      if (rc) return rc;
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
  launch_bwd_dense(QuatScaleForm{means, quats, scales, opacities},
                   PackedView{viewmats, Ks, N, C, width, height, 0.f, 0.f, eps2d, 0.f, flags}, indptr, nnz, gaussian_ids,
                   PackedCot{(const float4 *)g2d, v_comps, v_depths}, QuatScaleForm::Out{v_means, v_quats, v_scales},
                   as_stream(stream));
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
  launch_bwd_sparse(QuatScaleForm{means, quats, scales, opacities},
                    PackedView{viewmats, Ks, N, C, width, height, 0.f, 0.f, eps2d, 0.f, flags}, nnz, camera_ids,
                    gaussian_ids, PackedCot{(const float4 *)g2d, v_comps, v_depths},
                    QuatScaleForm::Out{v_means, v_quats, v_scales}, as_stream(stream));
  return check_launch("packed_bwd_sparse");
}

// ---- the covariance form: covars [N, 6] (upper triangle) in place of quats + scales
extern "C" int eg_packed_count_covars(const float *means, const float *covars, const float *viewmats, const float *Ks,
                                      int32_t N, int32_t C, int32_t width, int32_t height, float near_plane,
                                      float far_plane, float eps2d, float radius_clip, uint32_t flags,
                                      int32_t *block_base, int64_t *indptr, eg_stream_t stream) {
  EG_PACKED_SIZES(N, C, width, height);
  EG_REQUIRE(viewmats && Ks && indptr, "null pointer");
  EG_REQUIRE(N == 0 || (means && covars && block_base), "null pointer");
  launch_count(CovarForm{means, covars, nullptr},
               PackedView{viewmats, Ks, N, C, width, height, near_plane, far_plane, eps2d, radius_clip, flags},
               block_base, indptr, as_stream(stream));
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
  launch_write(CovarForm{means, covars, opacities},
               PackedView{viewmats, Ks, N, C, width, height, near_plane, far_plane, eps2d, radius_clip, flags},
               block_base, nnz,
               PackedOut{(float4 *)splat, radii, means2d, depths, conics, compensations, tiles_per_gauss,
                         (long long *)camera_ids, (long long *)gaussian_ids, tile_counts},
               as_stream(stream));
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
  launch_bwd_dense(CovarForm{means, covars, nullptr},
                   PackedView{viewmats, Ks, N, C, width, height, 0.f, 0.f, eps2d, 0.f, flags}, indptr, nnz, gaussian_ids,
                   PackedCot{(const float4 *)g2d, v_comps, v_depths}, CovarForm::Out{v_means, v_covars},
                   as_stream(stream));
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
  launch_bwd_sparse(CovarForm{means, covars, nullptr},
                    PackedView{viewmats, Ks, N, C, width, height, 0.f, 0.f, eps2d, 0.f, flags}, nnz, camera_ids,
                    gaussian_ids, PackedCot{(const float4 *)g2d, v_comps, v_depths}, CovarForm::Out{v_means, v_covars},
                    as_stream(stream));
  return check_launch("packed_bwd_sparse_covars");
}
