/*
 * edgegs.h -- C ABI of libedgegs.so, the MI355X (gfx950) edge-Gaussian rasterizer.
 *
 * This is the drop-in boundary for the ONE hot path of kunalchelani/EdgeGaussians: the call
 *     render, alpha, info = gsplat.rasterization(...)      reference edgegaussians/models/edge_gs.py:250-268
 * and its autograd backward (train_gaussians.py:101), plus the per-step glue around it
 * (edge_gs.py:278-324 loss, :603-613 absgrad, train_gaussians.py:104-106 Adam,
 * edge_gs.py:384-488,544-601 densify/cull).  The reference binds that path through Python
 * (`from gsplat import rasterization`, edge_gs.py:8); the binding a maintainer adds is the
 * ctypes stub in INTEGRATION.md (shipped as edgegaussians_amd/_lib.py + gsplat/__init__.py).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; plain pointers + sizes,
 *     no torch types; the library allocates nothing and keeps no state between calls -- with three stated
 *     exceptions, all measurement / communication plumbing and none on the default path: the HIP events of an open
 *     eg_timing_begin window, the per-wave profile buffer of the EG_FWD_PROF=1 debugging build path
 *     (eg_debug_fwd_profile), and the RCCL communicator handed to eg_dp_init (eg_train_steps_dp)
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t); no call synchronises
 *   - return 0 on success, a negative EG_ERR_* code otherwise (eg_last_error_string() explains)
 *   - fp32 arithmetic; indices int32; sort keys uint64 = (depth_bits << 32) | gaussian_id within
 *     a tile segment; isect ids int64 = (tile_id << 32) | depth_bits exactly as gsplat 1.0.0
 *   - N Gaussians, M tile intersections, T = tiles_x * tiles_y tiles of 16x16 pixels, one camera
 *     per call (the reference always passes C = 1, edge_gs.py:235-236; C > 1 is looped above)
 *
 * Packed per-Gaussian screen record ("splat", 8 floats, 32 B, one L2 sector pair):
 *     [0] x  [1] y  [2] conic a  [3] conic b  [4] conic c  [5] opacity*compensation
 *     [6] depth (fp32)  [7] radius (int32 bits; 0 = culled)
 * Packed per-Gaussian 2D gradient accumulator ("g2d", 8 floats, 32 B):
 *     [0] v_x [1] v_y [2] |v_x| [3] |v_y| [4] v_a [5] v_b [6] v_c [7] v_opacity_eff
 */
#ifndef EDGEGS_H
#define EDGEGS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *eg_stream_t; /* hipStream_t */

#define EG_OK 0
#define EG_ERR_ARG (-1)     /* bad argument (null pointer, negative size, unsupported channel count) */
#define EG_ERR_LAUNCH (-2)  /* hipGetLastError() after a launch */
#define EG_ERR_NODEVICE (-3)
#define EG_ERR_CAPACITY (-4) /* a result the entry itself read back does not fit the caller's buffers (eg_edge_sample) */

#define EG_TILE 16
#define EG_MAX_BATCH 8 /* views per eg_train_step_batched call */
#define EG_REWALK_SPECULATE (-2) /* rewalk_hint: do not launch the exact-stop re-walk; control word 3 reports a miss */
#define EG_FLAG_LOG_SCALES 1u      /* `scales` holds log-scales: exp() fused (edge_gs.py:253) */
#define EG_FLAG_LOGIT_OPACITIES 2u /* `opacities` holds logits: sigmoid() fused (edge_gs.py:254) */
#define EG_FLAG_ANTIALIASED 4u     /* rasterize_mode="antialiased" (edge_gs.py:50,266) */
#define EG_FLAG_ABSGRAD_WRITE 16u   /* eg_project_bwd: absgrads[g] = increment instead of += (data-parallel leg) */
#define EG_FLAG_FRONT_PREFIX 32u     /* eg_project_emit & co.: `ticket` is [T + 2] int32 and the scan of the last workgroup    \
                                      also leaves ticket[1 + t] = sum over the tiles before t of min(items, EG_FRONT_LARGE)  \
                                      and ticket[1 + T] = that sum over all tiles (dispatch classes of the forward on tile   \
                                      grids above 2560 tiles: the sort kernel then writes the item records front slices first) */
#define EG_FLAG_GRAD_ACCUM 64u       /* eg_project_bwd: v_means / v_quats / v_scales / v_opacities += instead of = (the sum over the \
                                      cameras of eg_project_bwd_cams) */
#define EG_FLAG_ORTHO 128u           /* orthographic camera (gsplat camera_model="ortho") on the operator path -- eg_project_fwd /       \
                                      _bwd and their _cams forms, eg_project_bwd_viewmats, eg_packed_count / _write / _bwd /        \
                                      _bwd_sparse and their _covars forms, eg_project_covars_{fwd,bwd}_cams_flags,                  \
                                      eg_project_covars_bwd_viewmats: mean2d = (fx x + cx, fy y + cy), J =                          \
                                      [[fx, 0, 0], [0, fy, 0]] (no division by z, no fov clamp; Ks in pixels per world unit), culls,  \
                                      depth = z and everything behind cov2d as under the pinhole.  The same bit goes to the forward   \
                                      and its backward.  Every other entry that takes caller flags refuses it with EG_ERR_ARG */
#define EG_FRONT_LARGE 9
#define EG_FLAG_TIGHT_TILES 8u     /* bin with the opacity-aware tile box (subset of gsplat's box that \
                                      drops only (Gaussian, tile) pairs contributing exactly nothing) */

const char *eg_last_error_string(void);
int eg_version(void);
/* number of gfx950 devices visible; <= 0 means the library cannot run (callers must fail loudly) */
int eg_device_count(void);

/* ---- G1: fully fused projection forward (replaces gsplat fully_fused_projection fwd)
 * Optional outputs may be NULL.  When tile_counts != NULL the per-tile intersection counts are
 * accumulated too (gsplat isect_tiles pass 1) -- tile_counts must be zeroed by the
 * caller once (eg_tile_emit returns it to zero every step).  g2d, when non-NULL, is zeroed for the
 * backward pass of this step. */
int eg_project_fwd(const float *means, const float *quats, const float *scales, const float *opacities,
                   const float *viewmat /*[16] row-major world->cam*/, const float *K /*[9]*/,
                   int32_t N, int32_t width, int32_t height, float near_plane, float far_plane,
                   float eps2d, float radius_clip, uint32_t flags,
                   float *splat /*[N,8]*/, int32_t *radii /*[N]|NULL*/, float *means2d /*[N,2]|NULL*/,
                   float *depths /*[N]|NULL*/, float *conics /*[N,3]|NULL*/, float *compensations /*[N]|NULL*/,
                   int32_t *tiles_per_gauss /*[N]|NULL*/, int32_t *tile_counts /*[T]|NULL*/,
                   float *g2d /*[N,8]|NULL*/, eg_stream_t stream);

/* ---- G1 + G2 + G3 for the fused training step: projection of raw parameters (log-scales, logits,
 * antialiased), per-tile counting with the opacity-aware exact tile test, AND the scan -- the last
 * workgroup to finish (device-scope ticket) produces offsets / item_offsets / total, which saves the
 * eg_tile_offsets launch.  tile_mask[N] receives each Gaussian's exact tile hits (bit mask over its
 * box, 0xffffffff = box larger than 32 tiles) for eg_tile_emit.  ticket: int32[1], zero-initialised
 * once by the caller (the kernel returns it to zero). */
int eg_project_bin(const float *means, const float *quats, const float *log_scales, const float *logit_opacities,
                   const float *viewmat, const float *K, int32_t N, int32_t width, int32_t height, uint32_t flags,
                   float *splat /*[N,8]*/, int32_t *tile_counts /*[T], zero on entry*/, uint32_t *tile_mask /*[N]*/,
                   int64_t capacity, int32_t *offsets /*[T+1]*/, int32_t *item_offsets /*[T+1]*/,
                   int32_t *total /*[4]*/, int32_t *ticket /*[1]*/, eg_stream_t stream);

/* ---- G2 (per-Gaussian part) on caller-supplied screen data: tiles_per_gauss + tile_counts from
 * (means2d, radii).  Used when projection ran elsewhere (parity tests feed oracle floats).  The general path's one
 * counting kernel (tiles of 8, 16 and 32 pixels: eg_tile_count_ts) at 16. */
int eg_tile_count(const float *means2d, const int32_t *radii, int32_t N, int32_t width, int32_t height,
                  int32_t *tiles_per_gauss /*[N]|NULL*/, int32_t *tile_counts /*[T]*/, eg_stream_t stream);

/* ---- G3+G6: exclusive scan of the per-tile counts -> isect_offsets[T+1] (offsets[T] = M), which is
 * gsplat's isect_offset_encode result.  tile_counts is left intact: eg_tile_emit
 * counts it back down to zero.  item_offsets[T+1] (may be NULL) is the exclusive scan of
 * ceil(count/128): the (tile, 128-Gaussian slice) work items of the compositing kernels.
 * total[4] = { M, overflow flag (M > capacity), number of items, largest tile population }.
 * The overflow flag is STICKY: every producer (this scan, eg_project_bin, eg_project_emit) only ever
 * raises total[1]; the caller zero-initialises it and clears it after reading, so one read after K
 * steps tells whether ANY of them dropped intersections. */
int eg_tile_offsets(const int32_t *tile_counts /*[T]*/, int32_t T, int64_t capacity,
                    int32_t *offsets /*[T+1]*/, int32_t *item_offsets /*[T+1]|NULL*/, int32_t *total /*[4]*/,
                    eg_stream_t stream);

/* ---- G4: emit one (depth_bits<<32 | gaussian_id) key per (Gaussian, tile) into that tile's
 * segment [offsets[t], offsets[t+1]) (order inside a segment arbitrary; eg_sort_pairs fixes it).  Two forms: from
 * (means2d, radii, depths) -- splat NULL; flags and tile_mask are not read -- by the general path's one emission kernel
 * (tiles of 8, 16 and 32 pixels: eg_tile_emit_sort_ts) at 16; from the splat records by a kernel of its own, which
 * alone knows the tight boxes and exact tile hits of the training step's classic layout. */
int eg_tile_emit(const float *means2d_or_null, const int32_t *radii_or_null, const float *depths_or_null,
                 const float *splat_or_null, uint32_t flags /*EG_FLAG_TIGHT_TILES needs splat*/,
                 int32_t N, int32_t width, int32_t height,
                 const int32_t *offsets /*[T+1]*/, int32_t *tile_counts /*[T]: counts on entry, zero on exit*/,
                 int64_t capacity, uint64_t *keys /*[capacity]*/,
                 const uint32_t *tile_mask /*[N]|NULL: exact tile hits left by eg_project_bin*/, eg_stream_t stream);

/* ---- G5: segmented sort -- every tile segment ascending by (depth bits, gaussian id), which equals
 * gsplat's stable radix sort on (tile, depth) of index-ordered emissions.  Writes the sorted
 * Gaussian ids (gsplat flatten_ids) and optionally the int64 isect ids (tile<<32 | depth_bits). */
int eg_sort_pairs(uint64_t *keys /*[capacity] in/out*/, const int32_t *offsets /*[T+1]*/, int32_t T,
                  int64_t capacity, int32_t *flatten_ids /*[capacity]*/, int64_t *isect_ids /*[capacity]|NULL*/,
                  int32_t max_tile_hint /*largest tile population seen so far, 0 = unknown: launch-shape hint
                  only (skips the idle launch of the large-tile variant), never affects the result*/,
                  eg_stream_t stream);

/* ---- segmented binning (training step): projection + binning in ONE pass.  Tile t owns the fixed
 * segment keys[t * seg_cap ... (t + 1) * seg_cap), so a Gaussian's keys are placed (one returning atomic
 * per workgroup and touched tile on tile_cursor[t]) without a count pass, a global scan of offsets or a
 * second (emit) kernel.  The last workgroup to finish (device-scope ticket) scans the populations:
 * item_first [T] (first 128-Gaussian slice of every tile) and total[4] = {M, overflow flag, items, largest
 * tile population}.  eg_sort_segments sorts every segment in place (same order as eg_sort_pairs) and
 * its one-workgroup-per-tile kernel writes the per-tile tables: tile_start/tile_end [T] (the keys),
 * item_end [T], item_tile [max_items] (owner of every item), and returns the cursors to zero.  A tile
 * above seg_cap (or more items than max_items) drops the excess and raises total[1].
 * eg_composite_fwd_segments = the slice-parallel eg_composite_fwd on those tables. */
int eg_project_emit(const float *means, const float *quats, const float *log_scales, const float *logit_opacities,
                    const float *viewmat, const float *K, int32_t N, int32_t width, int32_t height,
                    uint32_t flags /*must include EG_FLAG_TIGHT_TILES*/, float *splat /*[N,8]*/,
                    int32_t *tile_cursor /*[T] zero on entry*/, int32_t seg_cap, uint64_t *keys /*[T*seg_cap]*/,
                    int32_t *item_first /*[T]*/, int32_t max_items, int32_t *total /*[4]*/,
                    int32_t *ticket /*[1] zero-initialised once*/, eg_stream_t stream);
int eg_sort_segments(uint64_t *keys, int32_t *tile_cursor /*[T] in: populations, out: zero*/, int32_t T,
                     int32_t seg_cap, int32_t *flatten_ids /*[T*seg_cap]*/, int32_t *tile_start /*[T]*/,
                     int32_t *tile_end /*[T]*/, const int32_t *item_first /*[T]*/, int32_t *item_end /*[T]*/,
                     int32_t *item_tile /*[max_items]*/, int32_t max_items, int32_t max_tile_hint,
                     eg_stream_t stream);
int eg_composite_fwd_segments(const float *splat, const int32_t *tile_start, const int32_t *tile_end,
                              const int32_t *item_first, const int32_t *item_end, const int32_t *item_tile,
                              const int32_t *flatten_ids, int32_t width, int32_t height,
                              float *render /*[H,W]|NULL*/, float *alphas /*[H,W]|NULL*/,
                              int32_t *last_ids /*[H,W]|NULL*/, const float *gt, const float *wmap, float loss_scale,
                              float *vpix /*[H,W]|NULL*/, float *loss_out /*[1]*/, const int32_t *total,
                              int64_t max_items, void *workspace, float *gtstop /*[H,W,3]*/,
                              int32_t rewalk_hint, eg_stream_t stream);

/* ---- G7: alpha compositing forward (replaces gsplat rasterize_to_pixels fwd).
 * channels = 1 or 3.  colors == NULL means "all ones" (the reference's colours, edge_gs.py:247).
 * Fused weighted-L1 (edge_gs.py:279,288-324 in weight-map form): when wmap != NULL,
 * channel 0 is clamped to [0,1], loss_out[0] += sum_p wmap_p*|c0_p - gt_p| and
 * vpix[p] = loss_scale * wmap_p * sign(c0_p - gt_p) (the upstream gradient dL/dc0: v_render of
 * eg_composite_bwd_colors with one channel).
 * Slice-parallel mode (unit colours only): pass item_offsets + total from eg_tile_offsets, an upper
 * bound max_items >= total[2] (e.g. ceil(capacity/128) + T) and a workspace of
 * eg_composite_workspace_bytes(max_items, T) bytes; one workgroup runs per (tile, 128-Gaussian slice; an
 * empty tile owns one empty item).  The first eg_composite_workspace_ctl_bytes(max_items, T) bytes of the
 * workspace are control words (per-tile tickets, item flags and tags, the re-walk list counter): the caller ZEROES
 * them once when the workspace is allocated -- with these (max_items, T) -- and every call hands them back
 * zeroed.  With item_offsets == NULL (or per-Gaussian colours) one workgroup walks each tile.
 * When gtstop != NULL (the fused training step, whose backward reads nothing else) render, alphas,
 * last_ids and vpix may each be NULL and are then not materialised.  Without wmap the gtstop record carries
 * T_final itself (upstream gradient 1): the caller scales word 0 by its per-pixel upstream gradient before
 * eg_composite_bwd_footprint (what the gsplat-compatible operator's backward does). */
int64_t eg_composite_workspace_bytes(int64_t max_items, int64_t n_tiles);
int64_t eg_composite_workspace_ctl_bytes(int64_t max_items, int64_t n_tiles);
int eg_composite_fwd(const float *splat, const float *colors /*[N,channels]|NULL*/, int32_t channels,
                     const int32_t *offsets, const int32_t *flatten_ids, int32_t width, int32_t height,
                     float *render /*[H,W,channels]|NULL*/, float *alphas /*[H,W]|NULL*/,
                     int32_t *last_ids /*[H,W]|NULL*/, const float *gt /*[H,W]|NULL*/, const float *wmap /*[H,W]|NULL*/, float loss_scale,
                     float *vpix /*[H,W]|NULL*/, float *loss_out /*[1]|NULL*/,
                     const int32_t *item_offsets /*[T+1]|NULL*/, const int32_t *total /*[4]|NULL*/,
                     int64_t max_items, void *workspace,
                     float *gtstop /*[H,W,3] 32-bit words|NULL: {vpix * T_final (f32), id of the last contributor
                                     if the pixel's walk stopped on T <= 1e-4 else -1 (i32), that Gaussian's
                                     depth bits (u32)} for eg_backward_fused*/,
                     int32_t rewalk_hint /*how many (tile, slice) items needed the exact-stop re-walk lately: sizes that
                     kernel's grid, never affects the result; 0 = none seen, -1 = unknown.  The workspace's control
                     word [n_tiles + max_items + 2] holds the largest list length since the caller last zeroed it.
                     EG_REWALK_SPECULATE (-2): the caller bets that no pixel reaches the transmittance stop (true
                     until opacities have trained up) and the re-walk kernel is NOT launched; if a pixel does stop,
                     the sticky control word [n_tiles + max_items + 3] is raised and the results of that call are
                     INVALID -- the caller must check the word, restore its state and repeat the call with a
                     hint >= -1 (what EdgeTrainer's journal does), then zero the word*/,
                     eg_stream_t stream);

/* ---- G8: compositing backward (replaces gsplat rasterize_to_pixels bwd), order-dependent: general
 * colours, or unit colours when the caller wants their gradient.  channels = 1 or 3; colors == NULL means "all ones".
 * Accumulates into g2d with float atomics.  v_colors may be NULL.  Unit colours without a colour gradient take
 * eg_composite_bwd_footprint. */
int eg_composite_bwd_colors(const float *splat, const float *colors, int32_t channels,
                            const int32_t *offsets, const int32_t *flatten_ids, int32_t width, int32_t height,
                            const float *alphas, const int32_t *last_ids, const float *v_render,
                            const float *v_alphas, float *g2d, float *v_colors /*[N,channels]|NULL*/,
                            eg_stream_t stream);

/* ---- G9: fully fused projection backward (replaces gsplat fully_fused_projection bwd).
 * Consumes g2d; writes (not accumulates) gradients w.r.t. the SAME representation the forward
 * took (flags): v_means[N,3], v_quats[N,4], v_scales[N,3], v_opacities[N].
 * absgrads (edge_gs.py:603-613), when non-NULL: absgrads[g] += hypot(g2d[g][2], g2d[g][3]).
 * External mode (v_comps_ext != NULL; gsplat's autograd layout, where `opacities * compensations`
 * is a torch op between projection and compositing): dL/dcompensation is read from v_comps_ext[N],
 * g2d[.][7] is ignored and v_opacities may be NULL.  v_depths_ext[N] (may be NULL) adds dL/ddepth. */
int eg_project_bwd(const float *means, const float *quats, const float *scales, const float *opacities,
                   const float *viewmat, const float *K, int32_t N, int32_t width, int32_t height,
                   float eps2d, uint32_t flags, const float *splat, const float *g2d,
                   const float *v_comps_ext, const float *v_depths_ext,
                   float *v_means, float *v_quats, float *v_scales, float *v_opacities,
                   float *absgrads /*[N]|NULL*/, eg_stream_t stream);

/* hyper-parameters of the four torch.optim.Adam instances (train_utils.py:50-60) */
typedef struct {
  double lr_means, lr_scales, lr_quats, lr_opacities; /* doubles: the bias-corrected scalars are */
  double beta1, beta2, eps;                            /* formed in double like torch does, then cast */
  int32_t step;           /* 1-based step count shared by the four optimizers ... */
  int32_t group_steps[4]; /* ... unless overridden per optimizer (means, scales, quats, opacities):
                             0 = use `step`, > 0 = that optimizer's own count, < 0 = it does not step in
                             this call (the regulariser steps of train_gaussians.py:108-131 advance only
                             means / scales / quats, so the counts drift apart) */
} eg_adam_hyper;

/* ---- G8, footprint form (unit colours, fused path): every Gaussian's gradient is summed over its
 * own footprint in the gtstop image written by eg_composite_fwd (the unit-colour backward is
 * order-independent); a wavefront owns 8 Gaussians and deals its 64 lanes out in proportion to
 * their footprint sizes; the footprint is walked as a sheared box that follows the ellipse.  The g2d
 * record is WRITTEN -- no tile lists, no atomics, no zeroing of g2d, deterministic.
 * Footprints of any size are handled in the one launch (a screen-filling Gaussian takes the lanes of
 * its wavefront). */
int eg_composite_bwd_footprint(const float *splat, int32_t N, int32_t width, int32_t height,
                               const float *gtstop /*[H,W,3]*/, float *g2d /*[N,8] written*/,
                               eg_stream_t stream);

/* ---- whole backward of the fused path: eg_composite_bwd_footprint, then eg_project_bwd_adam
 * (hyper_host != NULL: absgrads accumulated, Adam applied) or eg_project_bwd (hyper_host == NULL:
 * gradients written to v_*, absgrads[g] += increment). */
int eg_backward_fused(float *means, float *quats, float *scales, float *opacities,
                      const float *viewmat, const float *K, int32_t N, int32_t width, int32_t height,
                      float eps2d, uint32_t flags, const float *splat, const float *gtstop, float *g2d,
                      float *v_means, float *v_quats, float *v_scales, float *v_opacities,
                      float *absgrads /*[N]|NULL*/, float *m, float *v,
                      const eg_adam_hyper *hyper_host /*NULL = write gradients*/, eg_stream_t stream);

/* ---- a6: absgrad accumulate on its own (edge_gs.py:607-613): absgrads += ||means2d.absgrad||_2 */
int eg_absgrad_accum(const float *means2d_absgrad /*[N,2]*/, int32_t N, float *absgrads, eg_stream_t stream);

/* ---- a7: the four torch.optim.Adam steps of train_gaussians.py:104-106 in one launch
 * (train_utils.py:50-60: betas 0.9/0.999, eps 1e-8, no weight decay, no amsgrad; torch 1.13
 * update order).  `step` is the 1-based step count shared by the four optimizers. */

int eg_adam_multi(float *means, float *scales, float *quats, float *opacities,
                  const float *g_means, const float *g_scales, const float *g_quats, const float *g_opacities,
                  float *m /*[N,11]: means3|scales3|quats4|opac1 blocks of N*dim*/, float *v /*same*/,
                  int32_t N, eg_adam_hyper hyper,
                  const float *absgrad_inc /*[N]|NULL*/, float *absgrads /*[N]|NULL: += absgrad_inc (the
                                             all-reduced increment of the data-parallel leg)*/,
                  eg_stream_t stream);

/* One torch.optim.Adam step on ONE flat fp32 tensor: what each of the reference's four optimizers does
 * (train_utils.py:50-60 builds them, train_gaussians.py:104-106 / 116-118 / 128-130 step them one by one) -- the
 * native leg of the drop-in optimizer class edgegaussians_amd/optim.py:Adam.  Same arithmetic as eg_adam_multi
 * (torch's update order, bias corrections formed in double on the host); `step` is the optimizer's 1-based count
 * AFTER this step.  zero_grad != 0 also clears `grad` (opt.zero_grad(set_to_none=False) in the same pass). */
int eg_adam_tensor(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, double lr, double beta1,
                   double beta2, double eps, int32_t step, int32_t zero_grad, eg_stream_t stream);

/* ---- Adam on the rows one call saw (csrc/adam_sparse.hip; edgegaussians_amd/optim.py: SparseAdam, SelectiveAdam).
 * Both: m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, p -= step_size m / (sqrt(v) + eps) -- eps on the UNCORRECTED
 * root, unlike eg_adam_tensor.  Rows that are not stepped are neither read nor written.  No float atomics: the same
 * bits every run.  Sizes are checked first (negative sizes, a width below 1, nnz * w or N * M at or above 2^31:
 * EG_ERR_ARG); nnz == 0 or N == 0 is EG_OK without a launch; then null pointers are refused by name.
 * eg_adam_sparse_rows: one torch.optim.SparseAdam step (torch/optim/_functional.py: sparse_adam) with
 *   step_size = lr sqrt(1 - beta2^step) / (1 - beta1^step) formed in double; `step` is the 1-based count AFTER this
 *   step.  param / exp_avg / exp_avg_sq [N, w]; values [nnz, w]; sorted_indices [nnz] ascending row indices; perm [nnz]
 *   the permutation of a STABLE sort that produced them (values row perm[k] belongs to sorted_indices[k]), or NULL when
 *   sorted_indices is the gradient's own coalesced index list (perm = identity).  The values of one row are added in
 *   fp32 in the order of the values tensor and the row is stepped once with the sum.  An index outside [0, N) and a
 *   perm entry outside [0, nnz) are skipped.  One thread walks a whole run of equal indices (see the file's header).
 * eg_adam_masked_rows: gsplat's SelectiveAdam step, step_size = lr (no bias correction).  param / grad / exp_avg /
 *   exp_avg_sq [N, M], visibility [N] bytes (a torch.bool tensor): rows with a non-zero byte step. */
int eg_adam_sparse_rows(float *param, float *exp_avg, float *exp_avg_sq, const float *values /*[nnz,w]*/,
                        const int64_t *sorted_indices /*[nnz]*/, const int64_t *perm /*[nnz] or NULL*/, int64_t nnz,
                        int64_t N, int32_t w, double lr, double beta1, double beta2, double eps, int32_t step,
                        eg_stream_t stream);
int eg_adam_masked_rows(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                        const uint8_t *visibility /*[N]*/, int64_t N, int32_t M, double lr, double beta1, double beta2,
                        double eps, eg_stream_t stream);

/* The same four Adam steps (identical arithmetic) fused with eg_project_emit of the view this rank rasterises NEXT:
 * the tail of a data-parallel step (after the all-reduce of the gradients), one launch and one read of the
 * parameters instead of two.  The step that follows passes eg_step_args.have_projection = 1.  flags as
 * eg_project_emit; buffers as eg_project_emit (segmented layout). */
int eg_adam_emit(float *means, float *scales, float *quats, float *opacities,
                 const float *g_means, const float *g_scales, const float *g_quats, const float *g_opacities,
                 float *m, float *v, int32_t N, eg_adam_hyper hyper, const float *absgrad_inc, float *absgrads,
                 const float *next_viewmat, const float *next_K, int32_t width, int32_t height, uint32_t flags,
                 float *splat, int32_t *tile_cursor, int32_t seg_cap, uint64_t *keys, int32_t *item_first,
                 int32_t max_items, int32_t *total, int32_t *ticket, eg_stream_t stream);

/* ---- fused G9 + absgrad + Adam: single-GPU training step tail (no gradient exchange needed). */
int eg_project_bwd_adam(float *means, float *quats, float *scales, float *opacities,
                        const float *viewmat, const float *K, int32_t N, int32_t width, int32_t height,
                        float eps2d, uint32_t flags, const float *splat, const float *g2d,
                        float *m, float *v, float *absgrads, eg_adam_hyper hyper, eg_stream_t stream);

/* ---- a8/a9: densify / cull row movement (edge_gs.py:384-488,544-576).
 * eg_compact: out[j] = in[i] for the j-th row i with keep[i] != 0 (stable); rows of `dim` floats.
 * `positions` is an exclusive scan of keep (int32[N]) computed by eg_mask_scan; returns nothing on host.
 * eg_append: out[n_old + k*n_sel + j] = in[sel_j] (+ noise) for copies k = 0..copies-1. */
int eg_mask_scan(const uint8_t *keep /*[N]*/, int32_t N, int32_t *positions /*[N]*/, int32_t *count /*[1]*/,
                 eg_stream_t stream);
int eg_compact_rows(const float *in, const uint8_t *keep, const int32_t *positions, int32_t N, int32_t dim,
                    float *out, eg_stream_t stream);
int eg_append_rows(const float *in, const uint8_t *sel, const int32_t *positions, int32_t N, int32_t n_sel,
                   int32_t dim, int32_t copies, const float *noise /*[copies*n_sel,dim]|NULL*/, float fill_zero,
                   float *out_tail /*[copies*n_sel, dim]*/, eg_stream_t stream);

/* ---- a10: cull_gaussians_not_projecting (edge_gs.py:578-601): hits[g] += 1 for every view whose
 * rounded projection of means[g] lands inside the image on an edge pixel. */
int eg_project_hits(const float *means, int32_t N, const float *P /*[V,3,4] = K @ viewmat[:3]*/, int32_t V,
                    const uint8_t *edge_masks /*[V,H,W]*/, int32_t width, int32_t height,
                    int32_t *hits /*[N] zeroed by caller*/, eg_stream_t stream);

/* ---- 8(f) rank 3 twin: filter_by_projection (edge_extraction/filtering.py:80-123): the post-hoc filter
 * of the edge-extraction stage.  visib[g] += edge_maps[v][round(v_g), round(u_g)] (the float edge
 * strength, not a mask) for every view v in which x = K (R X + t) lands inside the image; the caller
 * divides by V and thresholds (in float64, like numpy does there).  cams: [V, 21] floats = K (9, row-major) | R (9) | t (3). */
int eg_project_visibility(const float *means, int32_t N, const float *cams /*[V,21]*/, int32_t V,
                          const float *edge_maps /*[V,H,W]*/, int32_t width, int32_t height,
                          double *visib /*[N] f64 (the reference's accumulator type), zeroed by caller*/,
                          eg_stream_t stream);

/* ---- nearest neighbours + orientation regularisers (train_gaussians.py:108-131).
 * eg_knn: exact K <= 32 nearest neighbours (self excluded, ascending distance, ties by index) of N 3D
 * points on a uniform grid: origin/cell/dims chosen by the caller (bounding box of the points, a few
 * points per cell).  A wavefront answers a few cell-ordered queries one after the other: the rows of the query's
 * block of cells are dealt to groups of lanes, a lane evaluates one candidate per round, the K-best list is spread
 * over the lanes (insertion = one DPP shift, the same cost for every K).  Scratch: cell_of[N], cell_counts[C] (zero on entry, returned to zero),
 * cell_start[C+1], sorted[N,4] (the points in cell order: x y z index) with C = dims[0]*dims[1]*dims[2].  Replaces k_nearest_sklearn
 * (edge_gs.py:135-151). */
int eg_knn(const float *points /*[N,3]*/, int32_t N, int32_t K, const float *origin_host /*[3]*/, float cell,
           const int32_t *dims_host /*[3]*/, int32_t *cell_of, int32_t *cell_counts, int32_t *cell_start,
           float *sorted /*[N,4]*/, int32_t *out_idx /*[N,K]*/, float *out_d2 /*[N,K]|NULL squared distances*/,
           eg_stream_t stream);

/* eg_knn_auto: the grid search with the grid chosen on the DEVICE: bounding box by a reduction kernel, D x D x D
 * cubic cells with D = eg_knn_auto_dims(N, K) (a function of the sizes only, so the caller can size the scratch without
 * looking at the points) -- no host sync at all.  Scratch: cell_of[N], cell_counts[D^3] (zero on entry, returned to zero),
 * cell_start[D^3 + 1], sorted[N,4], grid_scratch (64 bytes, zero on entry, returned to zero).  Same result as eg_knn / eg_knn_small. */
int32_t eg_knn_auto_dims(int32_t N, int32_t K);
int eg_knn_auto(const float *points /*[N,3]*/, int32_t N, int32_t K, int32_t *cell_of, int32_t *cell_counts,
                int32_t *cell_start, float *sorted, void *grid_scratch, int32_t *out_idx /*[N,K]*/,
                float *out_d2 /*[N,K] or NULL*/,
                float *kth /*[N] or NULL: temporal coherence for callers that search the SAME (slowly moving) points
                             again and again -- on entry each point's K-th squared distance of the previous call
                             (0 = unknown), used times kth_slack as the entry bound of its list; on exit this call's.
                             Exactness does not depend on it: a bound that turns out too small costs a re-scan */,
                float kth_slack /* e.g. 1.2 */, eg_stream_t stream);

/* eg_knn_small: the same result (exact K <= 32 neighbours, self excluded, ascending (distance, index)) by
 * exhaustive search in ONE launch, for N <= 131072: no grid, no scratch.  A lane holds a candidate, a wavefront owns a
 * few queries whose K-best lists are spread over its lanes (one DPP shift per insertion).  The fastest entry up to
 * ~5 * 10^3 points; fastest when the rows are in spatial order (the scan starts at the queries' own rows). */
int eg_knn_small(const float *points /*[N,3]*/, int32_t N, int32_t K, int32_t *out_idx /*[N,K]*/,
                 float *out_d2 /*[N,K] or NULL*/, eg_stream_t stream);
/* ---- Cross-set nearest neighbour: for each of Q query points the nearest of M target points (the metrics of
 * eval_utils.py:400-509 -- accuracy / completeness / precision / recall -- and any pred <-> gt matching).  The queries
 * are a different set from the targets: self is NOT excluded (queries == targets finds every point itself, or a
 * lower-indexed duplicate, at distance 0).  d2 = fma(ez, ez, fma(ey, ey, ex * ex)), e = q - t, in fp32; candidates are
 * ordered by (d2, target index): among equal d2 the lowest index wins.  Both entries return the same bits.  Q >= 0,
 * M >= 1, both <= 2^29; Q == 0 launches nothing.
 * eg_nn_query_small: exhaustive, ONE launch, no scratch (Q * M <= 2^40).  A lane holds a candidate, a wavefront owns a
 * few queries; the running minimum over the (d2, index) key lives in the lanes and is folded by a DPP reduction. */
int eg_nn_query_small(const float *queries /*[Q,3]*/, int64_t Q, const float *targets /*[M,3]*/, int64_t M,
                      int32_t *out_idx /*[Q]*/, float *out_d2 /*[Q] squared distances*/, eg_stream_t stream);
/* eg_nn_query_auto: the same result on a uniform grid over the TARGETS chosen on the device as eg_knn_auto does
 * (bounding-box reduction, D = eg_knn_auto_dims(M, 1)) -- no host sync; queries may lie anywhere (outside the box they
 * are clamped into a boundary cell for the walk, the stopping test uses their real position).  Targets and queries are
 * counting-sorted by cell.  Scratch, sized from (Q, M) alone: cell_of[max(Q, M)], cell_counts[D^3] (zero on entry,
 * returned to zero), cell_start[D^3 + 1], sorted_targets[M,4], sorted_queries[Q,4], grid_scratch (64 bytes, zero on
 * entry, returned to zero). */
int eg_nn_query_auto(const float *queries /*[Q,3]*/, int64_t Q, const float *targets /*[M,3]*/, int64_t M,
                     int32_t *cell_of, int32_t *cell_counts, int32_t *cell_start, float *sorted_targets,
                     float *sorted_queries, void *grid_scratch, int32_t *out_idx /*[Q]*/, float *out_d2 /*[Q]*/,
                     eg_stream_t stream);
/* ---- Parametric edges -> points: the sampling in front of the reference's evaluation (eval_utils.py:120-398,
 * get_pred_points_and_directions[_from_dict]; eval.py --use_parametric_edges, fit_edges.py --save_sampled_points).
 * curves: Nc cubic Beziers, float64 control points [Nc,4,3]; lines: float64 end points [Nl,2,3].  Primitive order
 * everywhere: all curves, then all lines (eval.py:116).  Float64 throughout; fixed summation orders and no float
 * atomics, so two runs give the same bits.  Nc == 0 and Nl == 0 are both legal; nothing is launched for an empty side.
 *
 * eg_edge_sample_count: lengths[p] -- a curve's is the reference's composite Simpson sum (100 sub-intervals
 * [i/100, (i+1)/100], on each (|B'(a)| + 4 sum_odd + 2 sum_even + |B'(b)|) h / 3 with h = (b - a) / 100 and B' the true
 * Bezier derivative, eval_utils.py:120-165: one workgroup per curve), a line's is |p0 - p1|; counts[p] =
 * int(length // resolution) with Python's float floor division (the floor of the exact quotient, not floor(a / b));
 * offsets = the exclusive scan of counts (offsets[Nc + Nl] = total[0]), summed in int64.  total[0] = the number of
 * samples (saturated at INT32_MAX), total[1] = 1 when it exceeds INT32_MAX or `capacity` (capacity < 0: no limit of the
 * caller's), else 0.  No host sync: the caller reads total back. */
int eg_edge_sample_count(const double *curves /*[Nc,4,3]*/, int32_t Nc, const double *lines /*[Nl,2,3]*/, int32_t Nl,
                         double resolution /* > 0 */, int64_t capacity, double *lengths /*[Nc+Nl]*/,
                         int32_t *counts /*[Nc+Nl]*/, int32_t *offsets /*[Nc+Nl+1]*/, int32_t *total /*[2]*/,
                         eg_stream_t stream);
/* eg_edge_sample_emit: one thread per sample i < min(total[0], capacity): its primitive p by binary search in offsets,
 * k = i - offsets[p], n = counts[p], t = k * (1 / (n - 1)) as np.linspace(0, 1, n) (last sample exactly 1; n == 1:
 * t = 0); point = [t^3 t^2 t 1] M P (eval_utils.py:312-318) resp. (1 - t) p0 + t p1, in float64, rounded once to
 * float32.  directions (may be NULL): lines (p1 - p0) / (|p1 - p0| + 1e-6) (:389-391); curves, normalised in float64,
 * EG_EDGE_TANGENT_REFERENCE: the reference's A (3 t^2) + B (2 t) + C (:322-368; A t^2 + B t + C is the derivative, so
 * this is NOT the tangent away from t = 0), EG_EDGE_TANGENT_EXACT: the true derivative.  prim_ids (may be NULL): p.
 * `capacity` = the rows of the output buffers.  Nothing at all is written while total[1] is set. */
#define EG_EDGE_TANGENT_REFERENCE 0
#define EG_EDGE_TANGENT_EXACT 1
int eg_edge_sample_emit(const double *curves, int32_t Nc, const double *lines, int32_t Nl,
                        const int32_t *counts /*[Nc+Nl]*/, const int32_t *offsets /*[Nc+Nl+1]*/,
                        const int32_t *total /*[2]*/, int64_t capacity, int32_t tangent, float *points /*[capacity,3]*/,
                        float *directions /*[capacity,3]|NULL*/, int32_t *prim_ids /*[capacity]|NULL*/,
                        eg_stream_t stream);
/* eg_edge_sample: the two in one call for a caller with buffers of `capacity` rows.  It reads total[2] back into
 * total_host (ONE stream synchronise: not for graph capture) and launches exactly total[0] emission threads; when the
 * samples do not fit it emits nothing and returns EG_ERR_CAPACITY (total_host tells how many there are). */
int eg_edge_sample(const double *curves, int32_t Nc, const double *lines, int32_t Nl, double resolution,
                   int64_t capacity, int32_t tangent, double *lengths, int32_t *counts, int32_t *offsets,
                   int32_t *total /*[2] device*/, float *points, float *directions, int32_t *prim_ids,
                   int32_t *total_host /*[2] host*/, eg_stream_t stream);
/* compute_direction_loss (edge_gs.py:346-373): sum_out[0] += sum over the counted (i,k) of
 * |m_i . unit(mu_i - mu_nn(i,k))|; g_means += and g_quats = the gradient of that SUM.  top_k <= 0 or >= K:
 * every listed neighbour counts (loss = 1 - sum/(N K), the caller scales by -lambda/(N K)); 0 < top_k < K
 * ('enforce_half', :366-369, K = 2 k listed, top_k = k): only the top_k best-aligned neighbours of each
 * Gaussian count (loss = 1 - sum/(N top_k)).  K <= 32. */
int eg_direction_loss(const float *means, const float *quats, const float *log_scales,
                      const int32_t *nn_idx /*[N,K]*/, int32_t N, int32_t K, int32_t top_k,
                      float *g_means /*[N,3] accumulated*/, float *g_quats /*[N,4] written*/, float *sum_out,
                      eg_stream_t stream);
/* compute_ratio_loss (edge_gs.py:375-380): sum_out[0] += sum_i second/largest scale (loss = sum/N);
 * g_scales = gradient of the sum w.r.t. the log-scales. */
int eg_ratio_loss(const float *log_scales, int32_t N, float *g_scales /*[N,3] written*/, float *sum_out,
                  eg_stream_t stream);

/* One regulariser iteration of train_gaussians.py:108-131 as one native enqueue: loss ('direction' kind 0 /
 * 'ratio' kind 1), lambda = loss_sum * scale_factor / loss formed on the device, backward, and the Adam step of the
 * means / scales / quats optimizers (set hyper.group_steps[3] < 0: the opacity optimizer does not step there).
 * grads: [11 N] scratch in the block layout of eg_train_step's gradient buffer.  nn: neighbour table [N, nn_stride];
 * columns nn_offset .. nn_offset + K - 1 are used (the reference drops the nearest one, edge_gs.py:342).
 * loss_sum: device scalar or NULL (then loss_sum_host).  work: [2] floats; work[1] = the loss value afterwards. */
int eg_regulariser_step(int32_t kind, float *means, float *quats, float *log_scales, float *logit_opacities,
                        float *adam_m, float *adam_v, float *grads, int32_t N, const int32_t *nn, int32_t nn_stride,
                        int32_t nn_offset, int32_t K, int32_t top_k, const float *loss_sum, float loss_sum_host,
                        float scale_factor, float *work /*[2]*/, eg_adam_hyper hyper, eg_stream_t stream);
/* The same with ORDER-INDEPENDENT sums (data-parallel runs, SURVEY 8e: every rank must take bit-identical regulariser
 * steps): the neighbour gradients of the direction loss and the loss sums are accumulated with 64-bit fixed-point integer
 * atomics (2^-32 resolution) instead of float atomics, in `fixed` -- int64 [3 N + 1], zero on entry, handed back zeroed.
 * Agrees with eg_regulariser_step to ~1e-7 relative; equal bit for bit from run to run and from rank to rank. */
int eg_regulariser_step_fixed(int32_t kind, float *means, float *quats, float *log_scales, float *logit_opacities,
                              float *adam_m, float *adam_v, float *grads, int32_t N, const int32_t *nn, int32_t nn_stride,
                              int32_t nn_offset, int32_t K, int32_t top_k, const float *loss_sum, float loss_sum_host,
                              float scale_factor, float *work /*[2]*/, eg_adam_hyper hyper, int64_t *fixed /*[3 N + 1]*/,
                              eg_stream_t stream);

/* ---- the per-pixel loss weights of the 'bg_edge_ratio' strategy (edge_gs.py:298-314 in weight-map form) built on
 * the device: out[p] = [gt_p >= thr] / n_edge + [p among perm[0 .. n_sel)] / n_sel; perm = a random permutation
 * drawn by the caller (int64, distinct, taken modulo HW like the reference's unravel, :303-310). */
int eg_ratio_wmap(const float *gt /*[H*W]*/, float thr, int32_t n_edge, const int64_t *perm, int32_t n_sel, int32_t HW,
                  float *out /*[H*W]*/, eg_stream_t stream);

/* The same map with the sample drawn inside the kernel (one launch, no permutation buffer): the n_sel sampled
 * pixels are { p < n_bg : pi(p) < n_sel } for a pseudo-random permutation pi of [0, n_bg) keyed by `seed` (Feistel
 * network + cycle walking): exactly n_sel distinct pixels, uniformly distributed; a new seed gives a new sample. */
int eg_ratio_wmap_seeded(const float *gt /*[H*W]*/, float thr, int32_t n_edge, int32_t n_bg, int32_t n_sel,
                         uint64_t seed, int32_t HW, float *out /*[H*W]*/, eg_stream_t stream);
/* C of them by one native call: map c from gts[c] with (n_edge[c], n_bg[c], n_sel[c], seeds[c]) into out + c * HW (host
 * arrays; the same kernel, the same maps). */
int eg_ratio_wmaps_seeded(int32_t C, const float *const *gts, float thr, const int32_t *n_edge, const int32_t *n_bg,
                          const int32_t *n_sel, const uint64_t *seeds, int32_t HW, float *out /*[C,H*W]*/, eg_stream_t stream);

/* ---- whole training step for one view, enqueued from native code (train_gaussians.py:81-106):
 * project+count -> offsets -> emit -> sort -> composite+loss -> composite bwd -> project bwd
 * (+absgrad, +Adam when hyper != NULL).  All buffers caller-owned. */
typedef struct {
  /* trainable state, raw representation (log-scales, logit-opacities) */
  float *means, *quats, *log_scales, *logit_opacities;
  float *adam_m, *adam_v, *absgrads;
  int32_t N;
  /* view */
  const float *viewmat, *K, *gt, *wmap;
  int32_t width, height;
  float loss_scale; /* lambda_projection (train_gaussians.py:98) */
  /* workspace */
  float *splat, *g2d;
  int32_t *tile_counts, *offsets, *item_offsets, *total; /* [T], [T+1], [T+1], [4] */
  uint32_t *tile_mask;                                   /* [N] */
  int32_t *ticket;                                       /* [T + 2], zero-initialised once ([0]: the scan's ticket; [1..T+1]:
                                                            see EG_FLAG_FRONT_PREFIX, used on tile grids above 2560 tiles) */
  void *workspace;   /* eg_composite_workspace_bytes(max_items, T) bytes, control prefix zeroed at allocation */
  int64_t max_items; /* >= ceil(capacity/128) + T */
  uint64_t *keys;
  int32_t *flatten_ids;
  int64_t capacity;
  int32_t max_tile_hint;                /* see eg_sort_pairs; 0 = unknown */
  int32_t rewalk_hint;                  /* see eg_composite_fwd; 0 = none seen, < 0 = unknown */
  int32_t seg_cap;                      /* > 0: segmented binning (eg_project_emit ...): keys / flatten_ids are
                                           [T * seg_cap], offsets / item_offsets serve as tile_start / item_first */
  int32_t *tile_end, *item_end, *item_tile; /* [T], [T], [max_items]; used when seg_cap > 0 */
  float *render, *alphas, *vpix, *loss; /* [H,W], [H,W], [H,W], [1] accumulated */
  float *gtstop;                        /* [H,W,3] */
  int32_t *last_ids;
  /* gradient outputs (used when adam == NULL, e.g. before an RCCL all-reduce) */
  float *v_means, *v_quats, *v_scales, *v_opacities;
  const eg_adam_hyper *adam_host; /* NULL = write gradients instead of stepping */
  /* tail fusion across the step boundary (segmented layout, adam_host != NULL): when next_viewmat != NULL the
   * step's last kernel also projects + bins the NEXT view with the parameters it has just updated, and the next
   * eg_train_step call on that view passes have_projection = 1 to skip its own projection.  Any change to the
   * parameters or the buffers in between voids the projection (the caller then passes 0). */
  const float *next_viewmat, *next_K;
  int32_t have_projection;
  /* > 0: when pixels reach the transmittance stop (rewalk_hint != EG_REWALK_SPECULATE) the forward runs as ONE
   * chained kernel (slice products, phase B and the exact stop by decoupled look-back; same results as the
   * slice / combine / re-walk sequence).  The tag marks the items published in THIS call: it must differ from the
   * tags of all earlier calls on the same workspace since that workspace was zeroed (count up from 1;
   * eg_train_steps uses ws_tag .. ws_tag + K - 1).  0: the slice / combine / re-walk sequence. */
  int32_t ws_tag;
  /* optional (segmented layout): the sort kernel then also leaves one 16-byte record per item -- item_rec [max_items, 4]
   * = {tile, slice | slices << 16, ws_tag of this call, end of the tile's keys} (the slice's first key is tile * seg_cap +
   * 128 * slice), in the order the forward dispatches its workgroups in.  The record INDEX is not the item number -- the
   * hand-over storage is addressed through item_first -- and the table may have HOLES: the forward takes a record for
   * this call's iff word 2 equals ws_tag, so the table must be zeroed whenever the workspace is (tag wrap).  Tile grids of
   * of 512 .. 2560 tiles (eg_record_xcd_shift), one view per launch: XCD-aware placement -- workgroup b of a launch runs on XCD b % 8; the tiles are
   * dealt to the XCDs in 2 x 2-tile blocks, xcd = (block_x + 3 block_y) % 8, and XCD x's records sit at indices 8 k + x,
   * slices 0..3 of its tiles first, their deeper slices after them; the table spans 8 x the longest of the eight lists
   * (beyond max_items: the sticky overflow word).  Larger grids / batched launches: slices [0, 9) resp. [0, 4) of all
   * tiles first, then the deeper slices, no holes.  Grids of <= 2560 tiles, fused loss (wmap != NULL, no images wanted): an
   * EMPTY tile other than the last one has NO record -- its sort workgroup adds the background's loss term
   * sum_p wmap_p |gt_p| to the forward's partial sums and leaves; its gtstop pixels and its tile / item table entries are
   * not written (no Gaussian's footprint reaches them: the exact tile test is conservative), its one empty item stays in the
   * numbering.  The step
   * (no images wanted,
   * ws_tag > 0) runs the wave-autonomous forward, whose hand-over granules carry ws_tag: 1 <= ws_tag <= EG_MAX_WS_TAG,
   * different from the tag of every earlier call on this workspace since the workspace was last zeroed (the WHOLE
   * workspace must be zero before its first use; a caller that runs out of tags zeroes it again -- every 65 534
   * steps).  A wave of that kernel that polls a hand-over granule for tens of milliseconds without seeing it gives up
   * and raises bit 1 of control word 3 of the workspace (sticky, next to bit 0 = "a pixel stopped in speculative
   * mode"): the results of that call are void and the caller must say so.  Batched step: [C, max_items, 4]. */
  int32_t *item_rec;
  /* Round 6.  Inside a run of steps (adam_host, next_viewmat, segmented layout) on a tile grid of <= 2560 tiles (round 6: 2048 -> 2560, the reference's native 800 x 800 = 2500 tiles included) a scene of
   * up to 32768 Gaussians (eg_backward_is_fused) runs the step's backward as ONE kernel: every workgroup walks the
   * footprints of its 64 Gaussians (compositing VJP), then its first wave runs their projection VJP, absgrads, Adam and the
   * next view's projection + binning -- the same functions, the same arithmetic per Gaussian, bit-identical parameters; the
   * g2d record stays on chip (args.g2d is not written).  != 0: the two kernels of rounds 1-5 (footprint backward, then
   * projection backward + Adam + next projection), g2d written.  Everywhere else -- larger scenes, larger grids, no next
   * view, the gradient form -- the field is ignored (the two kernels run). */
  int32_t two_kernel_backward;
} eg_step_args;
#define EG_MAX_WS_TAG 0xfffe

/* (Segmented layout, tile grids of <= 2560 tiles: eg_train_step / eg_train_steps / eg_train_step_batched run the
 * projection kernels without their ticket + scan tail -- `ticket` is then unused -- let every tile's sort workgroup
 * form its item prefix from the cursors, and have the compositing kernel return the cursors to zero.  Same tables,
 * same results; the stand-alone entries eg_project_emit / eg_sort_segments / eg_composite_fwd_segments keep the
 * protocol described with them.) */
int eg_train_step(const eg_step_args *args_host, eg_stream_t stream);

/* 1 when a step of a run (adam_host, next_viewmat, segmented layout, two_kernel_backward == 0) on a scene of n_gaussians
 * and a grid of n_tiles tiles runs its backward as the ONE kernel described at eg_step_args.two_kernel_backward, else 0:
 * what a caller labels its measurements with (bench.py). */
int eg_backward_is_fused(int32_t n_gaussians, int32_t n_tiles);

/* 1 when the tile sort of a step (one view, segmented layout, "prefix here" grid) on a grid of n_tiles tiles with the
 * population hint max_tile_hint runs its 512-thread variant with TWO tiles per workgroup (grids of 513 .. 2048 tiles, hint
 * above 1536), else 0: a launch shape, never a result. */
int eg_sort_two_tiles_per_workgroup(int32_t n_tiles, int32_t max_tile_hint);

/* The XCD-aware placement of the item records (eg_step_args::item_rec) on a grid of n_tiles tiles with one view per launch:
 * tiles per block side = 2^result, 0 = dense records.  A caller sizes max_items for 8 x the longest of the eight lists. */
int eg_record_xcd_shift(int32_t n_tiles);

/* ---- K consecutive steps by one native call: step k = eg_train_step on view views_host[k] (taken out of the
 * [V,4,4] / [V,3,3] / [V,H,W] arrays) with weight map wmaps_host[k] and every active Adam step count of
 * args_host->adam_host advanced by k.  args_host's own viewmat / K / gt / wmap are ignored. */
int eg_train_steps(const eg_step_args *args_host, int32_t K, const int32_t *views_host,
                   const float *const *wmaps_host, const float *viewmats, const float *Ks, const float *gts,
                   eg_stream_t stream);

/* ---- S independent scenes side by side on ONE GPU (BASELINE configs[4], "one scene per GPU", with S of them sharing
 * a device: at the reference's sizes a single scene's dependent launches sit at their latency floor and leave most of
 * the chip idle).  K steps of every scene by one native call: scene s = eg_train_steps(args_host[s], K, views_host[s],
 * wmaps_host[s], viewmats[s], Ks[s], gts[s]) on streams[s] (distinct streams, distinct buffers: the scenes share
 * nothing, every scene's result equals its solo run).  n_threads host threads (1 .. S) share the scenes -- thread j
 * takes scenes j, j + n_threads, ... -- and walk them round-robin, step k of all their scenes before step k + 1 of any.
 * The reference trains one scene per process (train_gaussians.py:311); this is the throughput form of its 115-scan sweep.
 * Not inside an eg_timing_begin window.  Returns the first failing scene's code (eg_last_error_string names scene and step). */
int eg_train_steps_multi(int32_t S, const eg_step_args *const *args_host, int32_t K, const int32_t *const *views_host,
                         const float *const *const *wmaps_host, const float *const *viewmats, const float *const *Ks,
                         const float *const *gts, const eg_stream_t *streams, int32_t n_threads);

/* ---- C <= EG_MAX_BATCH views per launch sequence.  `args_host` as for eg_train_step
 * (segmented layout required; its viewmat / K / gt / wmap fields are ignored) with every per-view work buffer
 * holding C consecutive copies: splat, g2d [C,N,8]; tile_counts, offsets, tile_end, item_offsets, item_end [C,T];
 * item_tile [C,max_items]; keys, flatten_ids [C,T*seg_cap]; total [C,4]; ticket [C]; gtstop [C,H,W,3];
 * workspace = C blocks of eg_batched_workspace_stride(max_items, T) bytes (control prefix of each zeroed at
 * allocation).  render / alphas / last_ids / vpix are not materialised.  The gradients of the C views are
 * SUMMED (= what an all-reduce over C data-parallel ranks forms), absgrads += the C per-view increments, then
 * one Adam step (adam_host != NULL) or the summed gradients are written (v_means ...).  viewmats / Ks / gts /
 * wmaps: host arrays of C device pointers.  The reference steps after every view (train_gaussians.py:104-106):
 * this is a throughput mode with the semantics of data parallelism, on one GPU. */
int64_t eg_batched_workspace_stride(int64_t max_items, int64_t n_tiles);
int eg_train_step_batched(const eg_step_args *args_host, int32_t C, const float *const *viewmats,
                          const float *const *Ks, const float *const *gts, const float *const *wmaps,
                          eg_stream_t stream);

/* ---- C cameras per native call for the GENERAL operator path (gsplat.rasterization takes viewmats [C,4,4]; the reference
 * itself calls it with one camera, edge_gs.py:250-268).  Native loops over the per-camera entries above -- the same kernels,
 * the same results -- with the cameras' arrays as [C, ...] blocks, or as HOST arrays of C device pointers where the sizes
 * differ per camera (the binning arrays of M_c entries).  One native call per stage, one host read-back for all totals.
 * eg_tile_emit_sort_cams: per camera the binning step eg_packed_bin and eg_tile_emit_sort_ts run too (emission from
 * means2d / radii / depths, eg_sort_pairs), here without an id base and without the camera in the isect ids: the sorted
 * ids stay local to the camera. */
int eg_project_fwd_cams(const float *means, const float *quats, const float *scales, const float *opacities,
                        const float *viewmats /*[C,4,4]*/, const float *Ks /*[C,3,3]*/, int32_t N, int32_t C, int32_t width,
                        int32_t height, float near_plane, float far_plane, float eps2d, float radius_clip, uint32_t flags,
                        float *splat /*[C,N,8]*/, int32_t *radii, float *means2d, float *depths, float *conics,
                        float *compensations, int32_t *tiles_per_gauss /*[C,N] each, NULL ok*/,
                        int32_t *tile_counts /*[C,T]*/, eg_stream_t stream);
/* v_means [N,3], v_quats [N,4], v_scales [N,3] = SUM over the cameras (camera 0 writes, the others add) */
int eg_project_bwd_cams(const float *means, const float *quats, const float *scales, const float *opacities,
                        const float *viewmats, const float *Ks, int32_t N, int32_t C, int32_t width, int32_t height, float eps2d,
                        uint32_t flags, const float *splat /*[C,N,8]*/, const float *g2d /*[C,N,8]*/,
                        const float *v_comps_ext /*[C,N]*/, const float *v_depths_ext /*[C,N] or NULL*/, float *v_means,
                        float *v_quats, float *v_scales, eg_stream_t stream);
int eg_tile_offsets_cams(const int32_t *tile_counts /*[C,T]*/, int32_t T, int32_t C, int64_t capacity,
                         int32_t *offsets /*[C,T+1]*/, int32_t *item_offsets /*[C,T+1]*/, int32_t *total /*[C,4]*/,
                         eg_stream_t stream);
int eg_tile_emit_sort_cams(const float *means2d /*[C,N,2]*/, const int32_t *radii /*[C,N]*/, const float *depths /*[C,N]*/,
                           int32_t N, int32_t C, int32_t width, int32_t height, const int32_t *offsets /*[C,T+1]*/,
                           int32_t *tile_counts /*[C,T], returned to zero*/, const int64_t *M_host /*[C]*/,
                           uint64_t *const *keys, int32_t *const *flatten_ids, int64_t *const *isect_ids /*NULL ok*/,
                           const int32_t *max_tile_host /*[C] or NULL*/, eg_stream_t stream);
int eg_composite_fwd_cams(int32_t C, const float *splat /*[C,N,8]*/, int32_t N, const float *colors, int32_t colors_per_camera,
                          int32_t channels, const int32_t *const *offsets, const int32_t *const *flatten_ids, int32_t width,
                          int32_t height, float *render /*[C,H,W,channels]*/, float *alphas /*[C,H,W]*/,
                          int32_t *last_ids /*[C,H,W]*/, const int32_t *const *item_offsets, const int32_t *const *total,
                          const int64_t *max_items_host, void *const *workspace, float *gtstop /*[C,H,W,3] or NULL*/,
                          eg_stream_t stream);
int eg_composite_bwd_footprint_cams(const float *splat /*[C,N,8]*/, int32_t N, int32_t C, int32_t width, int32_t height,
                                    const float *gtstop /*[C,H,W,3]*/, float *g2d /*[C,N,8]*/, eg_stream_t stream);

/* ---- gsplat's render modes and backgrounds (rasterization(render_mode="D" | "ED" | "RGB+D" | "RGB+ED", backgrounds=...))
 * for C cameras, one launch each way (gridDim.y = camera) of the classic one-workgroup-per-tile kernels.  A rendered pixel
 * holds the `channels` colour channels (0, 1 or 3) and then, with depth != 0, the depth channel: the projection depth of
 * each Gaussian (word 6 of its splat record) composited like a colour.  channels == 0 (depth only) needs depth != 0;
 * with channels > 0, colors is required ([N, channels], or [C, N, channels] with colors_per_camera != 0): unlike
 * eg_composite_fwd, NULL does not mean unit colours.  backgrounds [C, channels] or NULL: pix[k] += T_final * bg[k] on
 * the colour channels (the depth channel's background is 0; ignored when channels == 0).  At least one of depth /
 * backgrounds is given (otherwise the call is eg_composite_fwd_cams).  offsets [C, T+1]: row c is camera c's scan,
 * local to its own list; flatten_ids: the C cameras' sorted lists one after the other (camera c's starts at the sum of
 * offsets[c'][T] over c' < c).  render [C, H, W, channels + (depth != 0)], alphas / last_ids [C, H, W] (last_ids local to
 * the camera's list, as eg_composite_fwd_cams writes them).
 * The backward takes the forward's alphas / last_ids and v_render [C, H, W, channels + (depth != 0)], v_alphas
 * [C, H, W] or NULL; it ACCUMULATES with float atomics into g2d [C, N, 8] (the layout of eg_composite_fwd's splat-side
 * record: v_means2d, |v_means2d|, v_conics, v_opacities), v_colors [C, N, channels] or NULL, and, with depth != 0,
 * v_depths [C, N] (dL/d(projection depth), for eg_project_bwd_cams): the caller zeroes them.  The background's own
 * gradient sum_pixels v_render * (1 - alpha) is left to the caller. */
int eg_composite_fwd_modes_cams(int32_t C, const float *splat /*[C,N,8]*/, int32_t N, const float *colors,
                                int32_t colors_per_camera, int32_t channels, int32_t depth,
                                const float *backgrounds /*[C,channels] or NULL*/, const int32_t *offsets /*[C,T+1]*/,
                                const int32_t *flatten_ids, int32_t width, int32_t height, float *render, float *alphas,
                                int32_t *last_ids, eg_stream_t stream);
int eg_composite_bwd_modes_cams(int32_t C, const float *splat /*[C,N,8]*/, int32_t N, const float *colors,
                                int32_t colors_per_camera, int32_t channels, int32_t depth,
                                const float *backgrounds /*[C,channels] or NULL*/, const int32_t *offsets /*[C,T+1]*/,
                                const int32_t *flatten_ids, int32_t width, int32_t height, const float *alphas,
                                const int32_t *last_ids, const float *v_render, const float *v_alphas /*or NULL*/,
                                float *g2d /*[C,N,8]*/, float *v_colors /*[C,N,channels] or NULL*/,
                                float *v_depths /*[C,N], with depth*/, eg_stream_t stream);

/* ---- colours of any channel count (rasterization(colors=[..., D]) with D other than 1 or 3), csrc/tiles.hip (the
 * kernels of eg_composite_{fwd,bwd}_ts_cams on 16-pixel tiles): the two entries above for ONE CHUNK of a wider tensor.  `channels` (1 .. 32) is the chunk width the caller declares; it
 * runs in the kernel instantiated for the next of 2, 4, 8, 16, 32, and `n_real` (1 .. channels) of its channels are real:
 * only those are loaded, stored or added to.  colors / v_colors / backgrounds point at the chunk's first channel inside
 * tensors whose rows are `color_stride` floats apart ([N, color_stride] or, with colors_per_camera != 0,
 * [C, N, color_stride]; backgrounds [C, color_stride]); render / v_render likewise with rows of `pixel_stride` floats
 * ([C, H, W, pixel_stride]).  With depth != 0 the depth channel is channel n_real of the chunk's pixel.  Unlike the mode
 * entries, neither depth nor backgrounds is required, colors is.  Forward: alphas and last_ids may be NULL (not
 * written: every chunk of a call computes the same).  Backward: accumulates like eg_composite_bwd_modes_cams; v_alphas
 * is given with ONE chunk of a call only (it would be counted once per chunk).  The sums of a wave end in the lanes
 * that add them: one atomic instruction per (wave, Gaussian). */
int eg_composite_fwd_wide_cams(int32_t C, const float *splat /*[C,N,8]*/, int32_t N, const float *colors,
                               int32_t colors_per_camera, int32_t channels, int32_t depth,
                               const float *backgrounds /*or NULL*/, const int32_t *offsets /*[C,T+1]*/,
                               const int32_t *flatten_ids, int32_t width, int32_t height, float *render,
                               float *alphas /*or NULL*/, int32_t *last_ids /*or NULL*/, int32_t n_real,
                               int32_t color_stride, int32_t pixel_stride, eg_stream_t stream);
int eg_composite_bwd_wide_cams(int32_t C, const float *splat /*[C,N,8]*/, int32_t N, const float *colors,
                               int32_t colors_per_camera, int32_t channels, int32_t depth,
                               const float *backgrounds /*or NULL*/, const int32_t *offsets /*[C,T+1]*/,
                               const int32_t *flatten_ids, int32_t width, int32_t height, const float *alphas,
                               const int32_t *last_ids, const float *v_render, const float *v_alphas /*or NULL*/,
                               float *g2d /*[C,N,8]*/, float *v_colors /*or NULL*/, float *v_depths /*[C,N], with depth*/,
                               int32_t n_real, int32_t color_stride, int32_t pixel_stride, eg_stream_t stream);

/* ---- N as the RECORD STRIDE of the four entries above, and packed records (N == EG_PACKED_STRIDE).
 * The mode and wide kernels use N for one thing only: camera c's block of splat, g2d, v_colors, v_depths (and of colors
 * with colors_per_camera != 0) starts c * N rows into the array, and flatten_ids index inside that block.  With
 * N == EG_PACKED_STRIDE (zero) every camera addresses the SAME arrays from row 0: splat / g2d [nnz, 8], colors / v_colors
 * [nnz, ...] (already gathered per pair, so colors_per_camera makes no difference), v_depths [nnz], and flatten_ids are
 * indices into the whole packed list of eg_packed_write (eg_packed_bin leaves them so).  offsets, the images and
 * backgrounds are per camera as before.  Nothing else in the entries reads N. */
#define EG_PACKED_STRIDE 0

/* ---- packed projection (rasterization(packed=True)), csrc/packed.hip: only the pairs (camera c, Gaussian n) whose
 * radius is positive after every cull -- exactly the set radii[c, n] > 0 of eg_project_fwd_cams with the same arguments,
 * with the same values bit for bit -- in ascending order of c * N + n.  nnz = number of pairs.
 * eg_packed_count: the culls of every pair, counted per workgroup of 256 Gaussians of one camera; block_base
 *   [C * ceil(N / 256)] int32 (the only scratch) receives the exclusive scan, indptr [C + 1] int64 the cameras' ranges
 *   (indptr[C] = nnz).  The caller reads indptr back (the one host synchronisation gsplat has for nnz, too).
 * eg_packed_write: recomputes the projection and writes pair p = its rank: splat [nnz, 8] (the record of the
 *   compositing kernels: x y a b c opacity*compensation depth radius), radii / depths / compensations /
 *   tiles_per_gauss [nnz], means2d [nnz, 2], conics [nnz, 3], camera_ids / gaussian_ids [nnz] int64, and adds the
 *   tile hits to tile_counts [C, T] (zeroed by the caller).  All outputs are required.  nnz == 0: nothing to do.
 * eg_packed_bin: emission (the general path's one kernel, as eg_tile_emit without splat) + eg_sort_pairs + the rebase
 *   of the sorted ids on every camera's range; indptr_host [C + 1], M_host [C] and
 *   max_tile_host [C] (or NULL) are HOST arrays, offsets [C, T + 1] from eg_tile_offsets_cams; keys / flatten_ids /
 *   isect_ids (NULL ok) hold sum(M_host) entries, camera c's from sum(M_host[:c]).  flatten_ids index the whole packed
 *   list; isect_ids carry the camera above the tile bits (camera << (32 + floor(log2(T)) + 1)).
 * eg_packed_bwd: v_means [N, 3], v_quats [N, 4], v_scales [N, 3] from g2d [nnz, 8] (layout of eg_composite_bwd_*'s
 *   g2d: words 0-1 v_means2d, 4-6 v_conics), v_comps [nnz] and v_depths [nnz] (or NULL).  One thread per Gaussian sums
 *   its pairs in camera order in registers and writes every row (zeros where no camera sees it): no atomics, the same
 *   bits on every run.  indptr: the DEVICE array eg_packed_count wrote.
 * eg_packed_bwd_sparse: the same VJP per pair without the sum: v_means [nnz, 3], v_quats [nnz, 4], v_scales [nnz, 3]
 *   (the values of sparse gradients whose indices are gaussian_ids). */
int eg_packed_count(const float *means, const float *quats, const float *scales, const float *opacities,
                    const float *viewmats /*[C,4,4]*/, const float *Ks /*[C,3,3]*/, int32_t N, int32_t C, int32_t width,
                    int32_t height, float near_plane, float far_plane, float eps2d, float radius_clip, uint32_t flags,
                    int32_t *block_base /*[C*ceil(N/256)]*/, int64_t *indptr /*[C+1]*/, eg_stream_t stream);
int eg_packed_write(const float *means, const float *quats, const float *scales, const float *opacities,
                    const float *viewmats, const float *Ks, int32_t N, int32_t C, int32_t width, int32_t height,
                    float near_plane, float far_plane, float eps2d, float radius_clip, uint32_t flags,
                    const int32_t *block_base, int64_t nnz, float *splat /*[nnz,8]*/, int32_t *radii, float *means2d,
                    float *depths, float *conics, float *compensations, int32_t *tiles_per_gauss, int64_t *camera_ids,
                    int64_t *gaussian_ids, int32_t *tile_counts /*[C,T]*/, eg_stream_t stream);
int eg_packed_bin(const float *means2d /*[nnz,2]*/, const int32_t *radii /*[nnz]*/, const float *depths /*[nnz]*/,
                  const int64_t *indptr_host /*[C+1]*/, int32_t C, int32_t width, int32_t height,
                  const int32_t *offsets /*[C,T+1]*/, int32_t *tile_counts /*[C,T], returned to zero*/,
                  const int64_t *M_host /*[C]*/, uint64_t *keys, int32_t *flatten_ids, int64_t *isect_ids /*NULL ok*/,
                  const int32_t *max_tile_host /*[C] or NULL*/, eg_stream_t stream);
int eg_packed_bwd(const float *means, const float *quats, const float *scales, const float *opacities,
                  const float *viewmats, const float *Ks, int32_t N, int32_t C, int32_t width, int32_t height, float eps2d,
                  uint32_t flags, const int64_t *indptr /*[C+1], device*/, int64_t nnz, const int64_t *gaussian_ids,
                  const float *g2d /*[nnz,8]*/, const float *v_comps /*[nnz]*/, const float *v_depths /*[nnz] or NULL*/,
                  float *v_means, float *v_quats, float *v_scales, eg_stream_t stream);
int eg_packed_bwd_sparse(const float *means, const float *quats, const float *scales, const float *opacities,
                         const float *viewmats, const float *Ks, int32_t N, int32_t C, int32_t width, int32_t height,
                         float eps2d, uint32_t flags, int64_t nnz, const int64_t *camera_ids, const int64_t *gaussian_ids,
                         const float *g2d /*[nnz,8]*/, const float *v_comps /*[nnz]*/, const float *v_depths /*[nnz] or NULL*/,
                         float *v_means /*[nnz,3]*/, float *v_quats /*[nnz,4]*/, float *v_scales /*[nnz,3]*/,
                         eg_stream_t stream);
/* The covariance form (rasterization(covars=[N,3,3], packed=True)): covars [N,6], the upper triangle (00, 01, 02, 11, 12,
 * 22) of the world covariance, in place of quats + scales.  The kept pairs are exactly the set radii[c, n] > 0 of
 * eg_project_covars_fwd_cams_flags with the same arguments, with its values bit for bit; flags: EG_FLAG_ANTIALIASED
 * (the record's opacity is opacities[n] * compensation, and v_comps is read) and EG_FLAG_ORTHO.  Arguments, layouts,
 * scratch, order and NULL rules as the four entries above; eg_packed_bin serves both forms.
 * eg_packed_bwd_covars: v_means [N, 3] and v_covars [N, 6] (an off-diagonal entry stands for both symmetric entries, as
 *   eg_project_covars_bwd_cams writes it), summed over the cameras in camera order in registers, every row written.
 * eg_packed_bwd_sparse_covars: the same VJP per pair: v_means [nnz, 3], v_covars [nnz, 6]. */
int eg_packed_count_covars(const float *means, const float *covars /*[N,6]*/, const float *viewmats /*[C,4,4]*/,
                           const float *Ks /*[C,3,3]*/, int32_t N, int32_t C, int32_t width, int32_t height,
                           float near_plane, float far_plane, float eps2d, float radius_clip, uint32_t flags,
                           int32_t *block_base /*[C*ceil(N/256)]*/, int64_t *indptr /*[C+1]*/, eg_stream_t stream);
int eg_packed_write_covars(const float *means, const float *covars /*[N,6]*/, const float *opacities,
                           const float *viewmats, const float *Ks, int32_t N, int32_t C, int32_t width, int32_t height,
                           float near_plane, float far_plane, float eps2d, float radius_clip, uint32_t flags,
                           const int32_t *block_base, int64_t nnz, float *splat /*[nnz,8]*/, int32_t *radii,
                           float *means2d, float *depths, float *conics, float *compensations,
                           int32_t *tiles_per_gauss, int64_t *camera_ids, int64_t *gaussian_ids,
                           int32_t *tile_counts /*[C,T]*/, eg_stream_t stream);
int eg_packed_bwd_covars(const float *means, const float *covars /*[N,6]*/, const float *viewmats, const float *Ks,
                         int32_t N, int32_t C, int32_t width, int32_t height, float eps2d, uint32_t flags,
                         const int64_t *indptr /*[C+1], device*/, int64_t nnz, const int64_t *gaussian_ids,
                         const float *g2d /*[nnz,8]*/, const float *v_comps /*[nnz]*/,
                         const float *v_depths /*[nnz] or NULL*/, float *v_means /*[N,3]*/, float *v_covars /*[N,6]*/,
                         eg_stream_t stream);
int eg_packed_bwd_sparse_covars(const float *means, const float *covars /*[N,6]*/, const float *viewmats,
                                const float *Ks, int32_t N, int32_t C, int32_t width, int32_t height, float eps2d,
                                uint32_t flags, int64_t nnz, const int64_t *camera_ids, const int64_t *gaussian_ids,
                                const float *g2d /*[nnz,8]*/, const float *v_comps /*[nnz]*/,
                                const float *v_depths /*[nnz] or NULL*/, float *v_means /*[nnz,3]*/,
                                float *v_covars /*[nnz,6]*/, eg_stream_t stream);

/* ---- tile sizes 8 and 32 (rasterization(tile_size=8 | 32)), csrc/tiles.hip.  Every entry above works on 16 x 16 pixel
 * tiles (EG_TILE); these take the tile size as an argument, with gsplat's meaning: tile_width = ceil(width / tile_size),
 * tile_height = ceil(height / tile_size), T their product, a Gaussian's tile box floor / ceil((x -+ r) / tile_size) in
 * fp32, a pixel walks the list of the tile_size x tile_size tile that contains it.  eg_tile_offsets_cams and
 * eg_sort_pairs depend on the tile size through T only and serve these entries as they are.  A tile size other than
 * the ones named, or bad sizes, return EG_ERR_ARG before anything is launched.
 * eg_tile_count_ts / eg_tile_emit_sort_ts (tile_size 8 or 32): eg_tile_count and eg_tile_emit + eg_sort_pairs for C
 *   cameras in one native call -- the very kernels of those entries (csrc/binning.hip: one counting and one emission
 *   kernel with the tile size as an argument), which 16 reaches through eg_tile_count, eg_tile_emit_sort_cams and
 *   eg_packed_bin.  ranges_host [C + 1] (HOST, ascending): camera c owns entries [ranges_host[c],
 *   ranges_host[c + 1]) of means2d / radii / depths / tiles_per_gauss -- {0, N, 2 N, ...} for the dense [C, N, ...]
 *   arrays of eg_project_fwd_cams (called with tiles_per_gauss and tile_counts NULL: its fused counting is 16-pixel),
 *   indptr for the packed lists of eg_packed_write.  tile_counts [C, T]: zeroed by the caller, accumulated by the count,
 *   returned to zero by the emission.  offsets [C, T + 1] from eg_tile_offsets_cams; M_host [C] and max_tile_host [C]
 *   (or NULL) are HOST arrays; keys / flatten_ids / isect_ids (NULL ok) hold sum(M_host) entries, camera c's from
 *   sum(M_host[:c]).  flatten_ids index inside the camera's range (rebase == 0) or the whole list (rebase != 0:
 *   ranges_host[c] added, as eg_packed_bin leaves them); isect_ids carry the camera above the tile bits
 *   (camera << (32 + floor(log2(T)) + 1)).
 * eg_composite_fwd_ts_cams / eg_composite_bwd_ts_cams (tile_size 8 or 32): eg_composite_{fwd,bwd}_wide_cams with the
 *   tile size behind `height` -- one chunk of `channels` <= 32 channels, n_real of them real, addressed by color_stride /
 *   pixel_stride inside full-width tensors, N the record stride (EG_PACKED_STRIDE for packed records), offsets
 *   [C, T + 1] and the cameras' lists one after the other in flatten_ids -- plus the DEPTH-ONLY form channels == 0,
 *   which needs depth != 0 and n_real == 0, stages no colours and ignores colors / backgrounds / v_colors (NULL ok);
 *   render / v_render then hold the depth in channel 0.  The same walk, hence the same alphas and last_ids for every
 *   chunking; the backward accumulates with one atomic instruction per (wave, Gaussian). */
int eg_tile_count_ts(const float *means2d /*[*,2]*/, const int32_t *radii, const int64_t *ranges_host /*[C+1]*/,
                     int32_t C, int32_t width, int32_t height, int32_t tile_size,
                     int32_t *tiles_per_gauss /*NULL ok*/, int32_t *tile_counts /*[C,T]*/, eg_stream_t stream);
int eg_tile_emit_sort_ts(const float *means2d /*[*,2]*/, const int32_t *radii, const float *depths,
                         const int64_t *ranges_host /*[C+1]*/, int32_t C, int32_t width, int32_t height,
                         int32_t tile_size, const int32_t *offsets /*[C,T+1]*/,
                         int32_t *tile_counts /*[C,T], returned to zero*/, const int64_t *M_host /*[C]*/, uint64_t *keys,
                         int32_t *flatten_ids, int64_t *isect_ids /*NULL ok*/,
                         const int32_t *max_tile_host /*[C] or NULL*/, int32_t rebase, eg_stream_t stream);
int eg_composite_fwd_ts_cams(int32_t C, const float *splat /*[C,N,8]*/, int32_t N, const float *colors /*NULL: channels == 0*/,
                             int32_t colors_per_camera, int32_t channels, int32_t depth,
                             const float *backgrounds /*or NULL*/, const int32_t *offsets /*[C,T+1]*/,
                             const int32_t *flatten_ids, int32_t width, int32_t height, int32_t tile_size, float *render,
                             float *alphas /*or NULL*/, int32_t *last_ids /*or NULL*/, int32_t n_real,
                             int32_t color_stride, int32_t pixel_stride, eg_stream_t stream);
int eg_composite_bwd_ts_cams(int32_t C, const float *splat /*[C,N,8]*/, int32_t N, const float *colors /*NULL: channels == 0*/,
                             int32_t colors_per_camera, int32_t channels, int32_t depth,
                             const float *backgrounds /*or NULL*/, const int32_t *offsets /*[C,T+1]*/,
                             const int32_t *flatten_ids, int32_t width, int32_t height, int32_t tile_size,
                             const float *alphas, const int32_t *last_ids, const float *v_render,
                             const float *v_alphas /*or NULL*/, float *g2d /*[C,N,8]*/, float *v_colors /*or NULL*/,
                             float *v_depths /*[C,N], with depth*/, int32_t n_real, int32_t color_stride,
                             int32_t pixel_stride, eg_stream_t stream);

/* ---- camera-pose gradient of the projection (gsplat's v_viewmats), csrc/viewmat_grad.hip: for every visible pair
 * (c, n), with v_t the cotangent of its camera-space mean (the v_depths term included), vW the cotangent of
 * W = R_c Rq diag(s) and M = Rq diag(s):  v_R[c][i][j] += v_t[i] mean[j] + sum_k vW[3i+k] M[j][k],  v_tr[c][i] += v_t[i];
 * v_viewmats [C, 4, 4] = [[v_R | v_tr], [0 0 0 0]] is written whole (a camera that sees nothing gets sixteen zeros).  Ks
 * gets no gradient.  Serves both layouts of the projection:
 *   dense   splat [C, N, 8] (eg_project_fwd_cams's record: the pair is visible when its radius word is positive),
 *           g2d [C, N, 8], v_comps [C, N], v_depths [C, N] or NULL as eg_project_bwd_cams takes them; indptr and
 *           gaussian_ids NULL, nnz 0;
 *   packed  splat NULL; indptr [C + 1] (the DEVICE array of eg_packed_count), nnz, gaussian_ids [nnz], g2d [nnz, 8],
 *           v_comps [nnz], v_depths [nnz] or NULL as eg_packed_bwd takes them.
 * scratch: scratch_blocks * C * 12 floats from the caller, scratch_blocks >= ceil(N / 256) (dense) or
 * ceil(min(nnz, N) / 256) (packed); with zero blocks it may be NULL.  One lane per pair, one 12-float partial per
 * workgroup, then one workgroup per camera folds the partials in a fixed order: no atomics, no host read-back, the same
 * bits on every run.  Null pointers and sizes (N < 0, C outside 1..65535, nnz < 0 or > N * C, a scratch too small) are
 * refused with EG_ERR_ARG before any device call. */
int eg_project_bwd_viewmats(const float *means, const float *quats, const float *scales, const float *opacities,
                            const float *viewmats, const float *Ks, int32_t N, int32_t C, int32_t width, int32_t height,
                            float eps2d, uint32_t flags, const float *splat /*[C,N,8] or NULL = packed*/,
                            const int64_t *indptr /*[C+1], device*/, int64_t nnz, const int64_t *gaussian_ids,
                            const float *g2d, const float *v_comps, const float *v_depths /*NULL ok*/,
                            float *scratch /*[C,scratch_blocks,12]*/, int32_t scratch_blocks,
                            float *v_viewmats /*[C,4,4]*/, eg_stream_t stream);
/* The covariance form: covars [N,6] (upper triangle) in place of quats + scales.  With cc = R_c S R_c^T the
 * camera-space covariance and v_cc its cotangent:  v_R[c] += v_t mean^T + (v_cc + v_cc^T) R_c S,  v_tr[c] += v_t.
 *   dense   radii [C, N] (eg_project_covars_fwd_cams_flags: the pair is visible when its radius is positive), g2d
 *           [C, N, 8] (words 0-1 v_means2d, 4-6 v_conics), v_comps [C, N], v_depths [C, N] or NULL; indptr and
 *           gaussian_ids NULL, nnz 0;
 *   packed  radii NULL; indptr, nnz, gaussian_ids, g2d, v_comps, v_depths as eg_packed_bwd_covars takes them.
 * flags: EG_FLAG_ANTIALIASED (v_comps is read; it may be NULL without) and EG_FLAG_ORTHO.  Scratch, sums, the zero bottom
 * row and the refusals as above; the fold kernel is the same. */
int eg_project_covars_bwd_viewmats(const float *means, const float *covars /*[N,6]*/, const float *viewmats,
                                   const float *Ks, int32_t N, int32_t C, int32_t width, int32_t height, float eps2d,
                                   uint32_t flags, const int32_t *radii /*[C,N] or NULL = packed*/,
                                   const int64_t *indptr /*[C+1], device*/, int64_t nnz, const int64_t *gaussian_ids,
                                   const float *g2d, const float *v_comps, const float *v_depths /*NULL ok*/,
                                   float *scratch /*[C,scratch_blocks,12]*/, int32_t scratch_blocks,
                                   float *v_viewmats /*[C,4,4]*/, eg_stream_t stream);

/* ---- the drop-in operator's fast path in two calls (edgegaussians_amd/rasterizer.py: the reference's own call of
 * gsplat.rasterization -- one camera, colours == 1 without grad, edge_gs.py:247-279 -- and its autograd backward).
 * eg_operator_fwd: projection + exact tile binning -> per-tile sort -> the training step's wave-autonomous forward in its
 * exact mode, with the accumulated-alpha image as output and T_final in the gtstop record (no fused loss); means2d is
 * copied out of the packed record; total[4] = 1 iff every entry of `colors` is 1, total[5] = control word 3 of the workspace
 * (bit 1: a look-back poll of the forward gave up: the outputs are void).  The per-call outputs (splat, alphas,
 * means2d, gtstop) are the caller's fresh tensors, everything else its cached work buffers; total is [8] int32
 * ([0..3] as everywhere, [1] the sticky overflow flag: the caller reads total[0..4] back ONCE after the call).
 * eg_operator_bwd: rec = gtstop with word 0 scaled by the upstream gradient v_alphas[p * v_stride] -> footprint backward
 * -> absgrad_out [N,2] = sum over pixels of |dL/dmean2d| (what the reference reads as means2d.absgrad, edge_gs.py:612)
 * -> (+ v_means2d when someone differentiates through info["means2d"]) -> projection backward. */
typedef struct {
  const float *means, *quats, *scales, *opacities, *colors; /* colors [N, color_channels] or NULL */
  int32_t color_channels;
  const float *viewmat, *K;
  int32_t N, width, height;
  uint32_t flags;                      /* EG_FLAG_ANTIALIASED | EG_FLAG_LOG_SCALES | EG_FLAG_LOGIT_OPACITIES */
  float *splat, *alphas, *means2d, *gtstop; /* [N,8], [H,W], [N,2]|NULL, [H,W,3] */
  int32_t *tile_counts, *tile_start, *tile_end, *item_first, *item_end, *item_tile, *item_rec;
  int32_t *total;                      /* [8] */
  int32_t *ticket;                     /* [T + 2], zero-initialised once */
  uint64_t *keys;
  int32_t *flatten_ids;
  int32_t seg_cap, max_tile_hint;
  int64_t max_items;
  void *workspace;                     /* eg_composite_workspace_bytes(max_items, T), zeroed at allocation */
  int32_t ws_tag;                      /* as eg_step_args.ws_tag: fresh per call, 1 .. EG_MAX_WS_TAG */
} eg_operator_args;
int eg_operator_fwd(const eg_operator_args *a, eg_stream_t stream);
int eg_operator_bwd(const eg_operator_args *a, const float *v_alphas, int64_t v_stride, float *rec /*[H,W,3] scratch*/,
                    float *g2d /*[N,8]*/, float *absgrad_out /*[N,2]|NULL*/, const float *v_means2d /*[N,2]|NULL*/,
                    float *v_means, float *v_quats, float *v_scales, float *v_opacities, eg_stream_t stream);

/* ---- spherical-harmonics colours (gsplat 1.0.0 `spherical_harmonics` and the sh_degree branch of `rasterization`),
 * csrc/sh.hip.  raw[c, n, :] = sum over k < (degree + 1)^2 of Y_k(dir[c, n] / |dir[c, n]|) * coeffs[(c,) n, k, :], with the
 * real spherical harmonics in the 3DGS / gsplat order and sign (k = l*l + l + m, Cartesian table times (-1)^m); degree 0..4,
 * K >= (degree + 1)^2 coefficient rows per Gaussian of which the rows above the degree's are ignored.  coeffs is [N, K, 3],
 * shared by the C cameras, or [C, N, K, 3] with coeffs_per_camera = 1 (0 or 1, nothing else).
 * ONE entry pair with a null-pointer switch for the directions: either dirs [C, N, 3] is given (any length, normalised
 * in the kernel; means and campos NULL), or dirs is NULL and dir[c, n] = means[n] - campos[c] (means [N, 3], campos [C, 3]).
 * masks [C, N] bytes or NULL: where 0 the colour is 0 and no gradient flows.  clamp != 0: colors = max(raw + 0.5, 0), and
 * the backward recomputes the gate (gradient passes where raw + 0.5 >= 0); clamp == 0: colors = raw.
 * eg_sh_bwd takes v_colors [C, N, 3] and WRITES (no accumulation, no zeroing by the caller) v_coeffs in the shape of
 * coeffs -- summed over the cameras when they share them, exact zeros in the rows above the degree's and where masked --
 * and, optionally, the gradient of the directions: v_dirs [C, N, 3] (with dirs) or v_means [N, 3], summed over the cameras
 * (with means / campos); NULL: not wanted.  One lane per Gaussian loops over the cameras: no atomics, bit-identical runs.
 * Every argument is checked before any HIP call; N == 0 returns EG_OK without a launch. */
int eg_sh_fwd(int32_t degree, int32_t K, int32_t C, int32_t N, const float *dirs /*[C,N,3] or NULL*/,
              const float *means /*[N,3] or NULL*/, const float *campos /*[C,3] or NULL*/, const float *coeffs,
              int32_t coeffs_per_camera, const uint8_t *masks /*[C,N] or NULL*/, int32_t clamp, float *colors /*[C,N,3]*/,
              eg_stream_t stream);
int eg_sh_bwd(int32_t degree, int32_t K, int32_t C, int32_t N, const float *dirs, const float *means, const float *campos,
              const float *coeffs, int32_t coeffs_per_camera, const uint8_t *masks, int32_t clamp,
              const float *v_colors /*[C,N,3]*/, float *v_coeffs, float *v_dirs /*[C,N,3] or NULL*/,
              float *v_means /*[N,3] or NULL*/, eg_stream_t stream);

/* ---- fused SSIM (the `fused_ssim` operation of 3DGS trainers), csrc/ssim.hip; edgegaussians_amd/ssim.py.
 * S[b, c] = A1 A2 / (B1 B2) of the five moments m1 = G*img1, m2 = G*img2, e11 = G*img1^2, e22 = G*img2^2,
 * e12 = G*(img1 img2), G* = the 11-tap Gaussian (sigma 1.5, normalised, fp32) along W then along H with zero padding of 5,
 * per (b, c) plane; s1 = e11 - m1^2, s2 = e22 - m2^2, s12 = e12 - m1 m2, A1 = 2 m1 m2 + C1, A2 = 2 s12 + C2,
 * B1 = m1^2 + m2^2 + C1, B2 = s1 + s2 + C2, C1 = 0.01^2, C2 = 0.03^2.  img1 / img2 are [B, C, H, W] fp32 read through
 * their own element strides (host arrays of four: b, c, h, w; >= 0; the caller guarantees that they address the tensor);
 * S and the derivative maps d_m1 (dS/dm1 at fixed e11, e22, e12), d_s1 = dS/ds1 and d_s12 = dS/ds12 are contiguous
 * [B, C, H, W]; the three maps are written when given and must be all given or all NULL (evaluation).
 * eg_ssim_bwd: v [B, C, H, W] contiguous, the cotangent of S;
 *   v_img1 = G*(v d_m1) + 2 img1 G*(v d_s1) + img2 G*(v d_s12), stored through img1's strides, every element once by
 *   one lane: no atomics, the same bits every run.  One launch each.  Null pointers, sizes < 1, B * C > 65535 planes,
 *   H > 65535 * 32 or W > 2^24 are refused with EG_ERR_ARG before any HIP call. */
int eg_ssim_fwd(const float *img1, const float *img2, int32_t B, int32_t C, int32_t H, int32_t W,
                const int64_t *strides1_host /*[4]*/, const int64_t *strides2_host /*[4]*/, float *S,
                float *d_m1 /*NULL ok*/, float *d_s1 /*NULL ok*/, float *d_s12 /*NULL ok*/, eg_stream_t stream);
int eg_ssim_bwd(const float *img1, const float *img2, int32_t B, int32_t C, int32_t H, int32_t W,
                const int64_t *strides1_host /*[4]*/, const int64_t *strides2_host /*[4]*/, const float *v,
                const float *d_m1, const float *d_s1, const float *d_s12, float *v_img1, eg_stream_t stream);

/* ---- the photometric loss as a scalar, csrc/ssim.hip; edgegaussians_amd/losses.py: photometric_loss.
 * out[0] = (1 - lambda) out[1] + lambda (1 - out[2]), out[1] = mean |img1 - img2| over B C H W, out[2] = the mean of
 * the map S of eg_ssim_fwd -- over all of it, or with valid != 0 over its crop by 5 on every side (H, W >= 11).  No map
 * is written: every workgroup (one per 32 x 32 tile of a plane) leaves its two partial sums in slab [slab_len >= 2 G],
 * G = ceil(W / 32) ceil(H / 32) B C, and a second launch adds them in index order: no atomics, the same bits every run.
 * d_m1, d_s1, d_s12 (all three or none) receive the derivative maps, zero outside the crop.  img1 / img2, their strides
 * and the limits on the sizes are those of eg_ssim_fwd.
 * eg_photometric_bwd, one launch: v_img1 = v [ (1 - lambda) / n sign(img1 - img2) - lambda / n_S (G*d_m1 + 2 img1
 *   G*d_s1 + img2 G*d_s12) ] through img1's strides, n = B C H W, n_S the number of map elements the mean ran over,
 *   v ONE float on the device (the cotangent of out[0]), sign(0) = 0. */
int eg_photometric_fwd(const float *img1, const float *img2, int32_t B, int32_t C, int32_t H, int32_t W,
                       const int64_t *strides1_host /*[4]*/, const int64_t *strides2_host /*[4]*/, int32_t valid,
                       float lambda, float *d_m1 /*NULL ok*/, float *d_s1 /*NULL ok*/, float *d_s12 /*NULL ok*/,
                       float *slab, int64_t slab_len, float *out /*[3]*/, eg_stream_t stream);
int eg_photometric_bwd(const float *img1, const float *img2, int32_t B, int32_t C, int32_t H, int32_t W,
                       const int64_t *strides1_host /*[4]*/, const int64_t *strides2_host /*[4]*/, int32_t valid,
                       float lambda, const float *v /*[1]*/, const float *d_m1, const float *d_s1, const float *d_s12,
                       float *v_img1, eg_stream_t stream);

/* ---- scalar pointwise image losses, csrc/losses.hip; edgegaussians_amd/losses.py.
 * t_p = w_p |c(x_p) - y_p|^q over a logical [B, C, H, W] problem (B C H W < 2^31): q = 1 or 2; c = clamp(., 0, 1) when
 * clamp != 0; w_kind 0: w_p = 1 (w NULL), 1: w fp32, 2: w a bool mask read as bytes.  x, y, w are each read through
 * their own four element strides (host arrays; >= 0, 0 = a broadcast dimension; the caller guarantees that they address
 * the tensors); work is assigned by the logical index, so the bits of the result do not depend on the strides.
 * eg_loss_fwd, two launches: every workgroup (1024 consecutive logical indices) leaves its partial sum -- and with a
 *   mask its count of selected elements, an integer -- in slab [slab_words >= G 4-byte words, 2 G with a mask],
 *   G = ceil(B C H W / 1024); the second launch adds them in index order.  out[0] = sum / D, out[1] = sum, out[2] = D;
 *   reduction 0: D = 1, 1: D = B C H W, 2 (w_kind 2 only): D = the count (0 selected elements: out[0] is nan).
 * eg_loss_bwd, one launch: g_p = (v / D) w_p q |c(x_p) - y_p|^(q - 1) sign(c(x_p) - y_p) [0 <= x_p <= 1 when clamped]
 *   through strides_g (>= 1 wherever the size is above 1); v ONE float on the device, D = fwd_out[2] of the forward;
 *   sign(0) = 0; exactly 0.0 where the mask is false, the weight is 0 or the gate is shut, whatever v / D is.
 * No atomics; nothing is read back to the host.  Bad arguments are refused with EG_ERR_ARG before any launch. */
int eg_loss_fwd(const float *x, const float *y, const void *w /*NULL iff w_kind 0*/, int32_t w_kind, int32_t B, int32_t C,
                int32_t H, int32_t W, const int64_t *strides_x_host /*[4]*/, const int64_t *strides_y_host /*[4]*/,
                const int64_t *strides_w_host /*[4], NULL ok with w_kind 0*/, int32_t q, int32_t clamp, int32_t reduction,
                void *slab, int64_t slab_words, float *out /*[3]*/, eg_stream_t stream);
int eg_loss_bwd(const float *x, const float *y, const void *w /*NULL iff w_kind 0*/, int32_t w_kind, int32_t B, int32_t C,
                int32_t H, int32_t W, const int64_t *strides_x_host /*[4]*/, const int64_t *strides_y_host /*[4]*/,
                const int64_t *strides_w_host /*[4], NULL ok with w_kind 0*/, int32_t q, int32_t clamp,
                const float *v /*[1]*/, const float *fwd_out /*[3]*/, float *g, const int64_t *strides_g_host /*[4]*/,
                eg_stream_t stream);

/* ---- bilateral grid: slice + apply, and the total-variation regulariser, csrc/bilagrid.hip;
 * edgegaussians_amd/bilagrid.py (the module docstring states the semantics, tests/bilagrid_util.py in float64).
 * grids [N, 12, L, Hg, Wg] fp32 contiguous (N 12 L Hg Wg < 2^31).  The samples are a logical [B, H, W] problem
 * (B H W < 2^31): rgb [B, H, W, 3] and xy [B, H, W, 2] are each read through their own four element strides (host
 * arrays: b, h, w, last; >= 0, 0 = a broadcast dimension; the caller guarantees that they address the tensors).
 * grid_idx: [B] int32 (idx_is_int64 0) or int64 (1) on the device, or NULL with B == N (image b uses grid b); the
 * caller checks its range, the kernels clamp it so that no access leaves the grids.
 * eg_bilagrid_slice_fwd, one launch: out [B, H, W, 3] contiguous.  While one grid, 48 L Hg Wg bytes, fits
 *   EG_BILAGRID_LDS_BUDGET the forward and the v_rgb kernel read it from a copy in LDS (persistent workgroups), above it
 *   from global memory: the same arithmetic and the same bits either way.  max_workgroups (>= 0; 0 = 256, one per
 *   CU) caps the persistent workgroups of the LDS kernels over all images -- each image gets at least one, and no
 *   workgroup fewer than 1024 samples -- so a caller can make one workgroup walk many blocks of samples; it changes
 *   no bit of out or v_rgb.  It is ignored above the budget.  B is not limited beyond B H W < 2^31.
 * eg_bilagrid_slice_bwd: v [B, H, W, 3] contiguous, the cotangent of out.  v_rgb [B, H, W, 3] contiguous (NULL: not
 *   wanted) is WRITTEN by one launch, a pure map: the same bits every run.  v_grids, in the shape of grids (NULL: not
 *   wanted), is ADDED TO with float atomics by one more launch: the caller zeroes it, and its bits depend on the order
 *   in which the adds arrive.  While one grid's gradient, 48 L Hg Wg bytes, fits EG_BILAGRID_LDS_BUDGET every
 *   workgroup sums its block of samples in LDS and flushes the non-zero words once; above it the samples add to
 *   global memory directly, combined per wave where a wave's samples share their cell.
 * eg_bilagrid_tv_fwd, two launches: out[0] = sum over the axes a of (L, Hg, Wg) with n_a > 1 of
 *   mean((x[.. i + 1 ..] - x[.. i ..])^2), the mean over all N 12 (n_a - 1) (the other two sizes) differences; slab
 *   [slab_len >= ceil(N 12 L Hg Wg / 1024)] holds one partial per workgroup, added in index order by the second launch.
 * eg_bilagrid_tv_bwd, one launch: v_grids = v[0] times the gradient of that value, every cell from its <= 6 neighbours;
 *   v ONE float on the device.  No atomics in either: the same bits every run.
 * Bad arguments are refused with EG_ERR_ARG before any launch; nothing is read back to the host. */
#define EG_BILAGRID_LDS_BUDGET (96 * 1024) /* bytes of LDS the scatter may take: the 8 x 16 x 16 grid exactly */
int eg_bilagrid_slice_fwd(const float *grids, int32_t N, int32_t L, int32_t Hg, int32_t Wg, const float *rgb,
                          const float *xy, const void *grid_idx /*NULL ok with B == N*/, int32_t idx_is_int64, int32_t B,
                          int32_t H, int32_t W, const int64_t *strides_rgb_host /*[4]*/,
                          const int64_t *strides_xy_host /*[4]*/, int32_t max_workgroups /*0: one per CU*/, float *out,
                          eg_stream_t stream);
int eg_bilagrid_slice_bwd(const float *grids, int32_t N, int32_t L, int32_t Hg, int32_t Wg, const float *rgb,
                          const float *xy, const void *grid_idx /*NULL ok with B == N*/, int32_t idx_is_int64, int32_t B,
                          int32_t H, int32_t W, const int64_t *strides_rgb_host /*[4]*/,
                          const int64_t *strides_xy_host /*[4]*/, int32_t max_workgroups /*0: one per CU*/,
                          const float *v, float *v_rgb /*NULL ok*/, float *v_grids /*NULL ok*/, eg_stream_t stream);
int eg_bilagrid_tv_fwd(const float *grids, int32_t N, int32_t L, int32_t Hg, int32_t Wg, float *slab, int64_t slab_len,
                       float *out /*[1]*/, eg_stream_t stream);
int eg_bilagrid_tv_bwd(const float *grids, int32_t N, int32_t L, int32_t Hg, int32_t Wg, const float *v /*[1]*/,
                       float *v_grids, eg_stream_t stream);

/* ---- native data-parallel run (edgegaussians_amd/dist.py drives it).  RCCL is dlopen'ed from
 * `librccl_path` (NULL / "": "librccl.so" by the loader's search path) -- the library PyTorch ships, so that the process
 * holds ONE RCCL -- and the communicator is created from a 128-byte ncclUniqueId: rank 0 calls eg_dp_unique_id, the
 * ranks exchange the bytes (torch.distributed broadcast), every rank calls eg_dp_init on ITS device.  One communicator
 * per process (library state: see the conventions above).  eg_dp_world() = its size, 0 without one. */
int eg_dp_unique_id(const char *librccl_path, void *id_out_host /*128 bytes*/);
int eg_dp_init(const char *librccl_path, const void *id_host /*128 bytes*/, int32_t rank, int32_t world);
int eg_dp_world(void);
int eg_dp_shutdown(void);
/* the communicator's size as RCCL reports it (ncclCommCount): what bench.py puts on its line as the proof that RCCL saw
 * N ranks; 0 without a communicator, negative on an error */
int eg_dp_comm_count(void);
/* test / measurement switch.  on > 0 makes eg_train_steps_dp issue its [12 N] ncclAllReduce through a ONE-rank
 * communicator too (a sum over one rank is the identity, the run skips it by default: RCCL does it with copy-engine blits
 * that stall the stream).  on < 0 (round 6, MEASUREMENT ONLY): the collective is left out with N ranks as well -- every
 * rank then steps on its own view's gradient, the replicas DIVERGE and the run is no longer the reference's data-parallel
 * step; bench.py times one such window after all its valid ones ("step time with the collective compiled out") so that a
 * scaling curve separates RCCL's latency from everything else.  0: default.  Reset by eg_dp_shutdown. */
int eg_dp_force_all_reduce(int32_t on);
/* [12 N] gradient collectives issued by eg_train_steps_dp since eg_dp_init (and the floats they carried) */
int64_t eg_dp_grad_all_reduces(int64_t *floats_out_host /*NULL ok*/);
/* measurement aid: HIP events on the launch stream around the [12 N] collective of the next n_steps steps of
 * eg_train_steps_dp; _end synchronises once: mean / max microseconds the collective occupied the launch stream
 * (everything in it is exposed at one view per rank), number of collectives timed */
int eg_dp_comm_timing_begin(int32_t n_steps);
int eg_dp_comm_timing_end(float *mean_us_host, float *max_us_host, int32_t *n_out_host);
/* in-place sum over the ranks of n floats on `stream` (small collectives that ride the same communicator) */
int eg_dp_all_reduce(float *buf, int64_t n, eg_stream_t stream);
/* measurement aid: mean HOST microseconds per step that eg_train_steps_dp spent enqueueing {the gradient step's kernels,
 * ncclAllReduce, Adam + next projection} since the last call; returns the number of steps averaged */
int64_t eg_dp_host_profile(double *us_out_host /*[3]*/);
/* K consecutive view-sharded optimizer steps by ONE native call; per step: eg_train_step in its gradient form ->
 * ncclAllReduce(sum, fp32) of the fused [12 N] gradient buffer on the launch stream -> eg_adam_emit (the four Adam steps
 * on the reduced gradient + projection / binning of this rank's next view; eg_adam_multi when there is none).  `a`: step
 * 0 as for eg_train_step with adam_host == NULL and v_means / v_quats / v_scales / v_opacities / absgrads the blocks of
 * ONE contiguous buffer [means 3N | quats 4N | log-scales 3N | logit-opacity N | absgrad increment N]; its view inputs
 * are ignored: step k takes view views_host[k] of the [V, ...] arrays and weight map wmaps_host[k].  hyper: step 0's
 * Adam state (counts advance by k); absgrads: the accumulator that receives the reduced increment; next_view_after: the
 * view this rank rasterises in the step after the run (its projection rides in the last Adam launch; the caller then
 * passes have_projection = 1), or < 0.  Same results as the three calls enqueued one by one. */
int eg_train_steps_dp(const eg_step_args *a, const eg_adam_hyper *hyper, float *absgrads, int32_t K,
                      const int32_t *views_host, const float *const *wmaps_host, const float *viewmats /*[V,4,4]*/,
                      const float *Ks /*[V,3,3]*/, const float *gts /*[V,H,W]*/, int32_t next_view_after,
                      eg_stream_t stream);

/* ---- gsplat's functional API (csrc/functional.hip; edgegaussians_amd/functional.py).  Every entry is asynchronous on
 * `stream`, rejects null pointers (other than the ones named) and bad sizes with EG_ERR_ARG before any device call, and
 * uses no atomics: the same bits every run.  A [N,6] tensor holds the upper triangle (00, 01, 02, 11, 12, 22) of a
 * symmetric matrix; in a GRADIENT of that shape an off-diagonal entry stands for both symmetric entries (what autograd
 * gives through "build the matrix, select the upper triangle" / "place the six numbers into the symmetric matrix").
 *
 * eg_quat_scale_to_covar_preci_fwd: covars = R diag(s^2) R^T, precis = R diag(1 / s^2) R^T from quats [N,4] (w, x, y, z;
 *   normalised inside with rsqrtf of the squared norm) and scales [N,3]; either output NULL = not computed; triu != 0:
 *   [N,6], else [N,3,3].  _bwd: v_covars / v_precis in the same layout (either NULL) -> v_quats [N,4], v_scales [N,3],
 *   every row written.  N == 0: nothing to do. */
int eg_quat_scale_to_covar_preci_fwd(const float *quats, const float *scales, int32_t N, int32_t triu,
                                     float *covars /*NULL ok*/, float *precis /*NULL ok*/, eg_stream_t stream);
int eg_quat_scale_to_covar_preci_bwd(const float *quats, const float *scales, int32_t N, int32_t triu,
                                     const float *v_covars /*NULL ok*/, const float *v_precis /*NULL ok*/,
                                     float *v_quats, float *v_scales, eg_stream_t stream);
/* gsplat fully_fused_projection(means, covars = [N,6], quats = None, scales = None, packed = False) for C cameras:
 * cov2d = J Rv S Rv^T J^T, everything else as eg_project_fwd_cams (near / far cull, the 1.3 tan-fov clamp, + eps2d,
 * det <= 0 cull, compensation, radius, radius_clip, off-screen cull).  radii int32 [C,N], means2d [C,N,2], depths
 * [C,N], conics [C,N,3], compensations [C,N] or NULL; a culled pair has radius 0 and zeros in every float output.
 * _bwd: v_means [N,3] and v_covars [N,6], the sum over the cameras with radii > 0 in camera order, every row written;
 * v_depths and v_compensations (gsplat's 0.5 v / (comp + 1e-6)) may be NULL.  N == 0: nothing to do. */
int eg_project_covars_fwd_cams(const float *means, const float *covars, const float *viewmats, const float *Ks,
                               int32_t N, int32_t C, int32_t width, int32_t height, float near_plane, float far_plane,
                               float eps2d, float radius_clip, int32_t *radii, float *means2d, float *depths,
                               float *conics, float *compensations /*NULL ok*/, eg_stream_t stream);
int eg_project_covars_bwd_cams(const float *means, const float *covars, const float *viewmats, const float *Ks,
                               int32_t N, int32_t C, int32_t width, int32_t height, float eps2d, const int32_t *radii,
                               const float *v_means2d, const float *v_depths /*NULL ok*/, const float *v_conics,
                               const float *v_compensations /*NULL ok*/, float *v_means, float *v_covars,
                               eg_stream_t stream);
/* The same pair with a camera model: flags = 0 (pinhole: the kernels and bits of the pair above) or EG_FLAG_ORTHO; any
 * other bit is refused.  Arguments, culls, layouts and NULL rules as above. */
int eg_project_covars_fwd_cams_flags(const float *means, const float *covars, const float *viewmats, const float *Ks,
                                     int32_t N, int32_t C, int32_t width, int32_t height, float near_plane,
                                     float far_plane, float eps2d, float radius_clip, int32_t *radii, float *means2d,
                                     float *depths, float *conics, float *compensations /*NULL ok*/, uint32_t flags,
                                     eg_stream_t stream);
int eg_project_covars_bwd_cams_flags(const float *means, const float *covars, const float *viewmats, const float *Ks,
                                     int32_t N, int32_t C, int32_t width, int32_t height, float eps2d,
                                     const int32_t *radii, const float *v_means2d, const float *v_depths /*NULL ok*/,
                                     const float *v_conics, const float *v_compensations /*NULL ok*/, float *v_means,
                                     float *v_covars, uint32_t flags, eg_stream_t stream);
/* gsplat isect_offset_encode on a caller's SORTED isect ids [M] (camera << (32 + tile_bits) | tile << 32 | depth bits,
 * tile_bits = floor(log2(T)) + 1, T = tile_width * tile_height): offsets [C, T] int32, offsets[c, t] = number of
 * entries whose (camera, tile) is below (c, t).  M == 0 (isect_ids may be NULL): all zeros.  No host read-back. */
int eg_isect_offset_encode(const int64_t *isect_ids, int64_t M, int32_t C, int32_t tile_width, int32_t tile_height,
                           int32_t *offsets, eg_stream_t stream);

/* ---- per-pixel intersection lists (csrc/indices.hip; functional.rasterize_to_indices_in_range / accumulate).  No
 * atomics anywhere: the same bits every run.  Null pointers (other than the ones named) and bad sizes are refused with
 * EG_ERR_ARG before any device call.
 * eg_indices_count / eg_indices_write (tile_size 8, 16 or 32): two passes of ONE walk, the forward walk of the
 *   compositing kernels (same sigma, threshold skip, alpha cap 0.999, 1/255 cut, stop BEFORE the entry that would take
 *   T to <= 1e-4).  A tile's list is cut into batches of tile_size^2 entries; pixel p of camera c starts from
 *   transmittances[c, p] and walks the batches b, range_start <= b < range_end, of its tile.  means2d [C,N,2], conics
 *   [C,N,3], opacities [C,N]; offsets [C, T + 1] local to each camera's list and the cameras' lists one after the other
 *   in flatten_ids [n_isects], whose values are Gaussian indices in [0, N) (what eg_composite_*_wide_cams take); a
 *   tile's range is clamped into [0, n_isects] before any load.  The count writes counts [C * H * W] (every pixel);
 *   the caller scans them into starts [C * H * W] (exclusive, 64-bit) and their sum `total`; the write stores row
 *   starts[p] + k of gaussian_ids / pixel_ids (i * width + j) / camera_ids [total] for the k-th entry pixel p takes,
 *   and never a row outside [0, total).  C * H * W == 0 or N == 0: EG_OK without a launch.
 * eg_accumulate_fwd / eg_accumulate_bwd: per pixel p the entries k of [starts[p], starts[p] + counts[p]) (clamped into
 *   [0, M]), in order: T_k = prod over the earlier k' of (1 - alpha[k']), w_k = alpha[k] T_k, render[p, ch] = sum w_k
 *   feat[k, ch] for ONE chunk of `channels` <= 32 channels addressed by feat_stride / pixel_stride inside full-width
 *   tensors, alphas[p] = sum w_k (NULL: not wanted), T_k [M] (NULL: not wanted).  The backward takes T_k back and
 *   walks the segments in reverse without dividing by (1 - alpha): v_feat[k, ch] = w_k v_render[p, ch] (written, same
 *   stride as feat), v_alpha[k] = (add ? v_alpha[k] : 0) + T_k (s_k - S_k) with s_k = feat[k] . v_render[p] +
 *   v_alphas[p] (NULL: 0) and S_k the suffix sum of alpha_j s_j prod_{k<k'<j} (1 - alpha_k').  One lane owns one
 *   pixel's segment.  P == 0: EG_OK without a launch. */
int eg_indices_count(int32_t C, int32_t N, const float *means2d, const float *conics, const float *opacities,
                     const float *transmittances /*[C,H,W]*/, const int32_t *offsets /*[C,T+1]*/,
                     const int32_t *flatten_ids, int64_t n_isects, int32_t width, int32_t height, int32_t tile_size,
                     int32_t range_start, int32_t range_end, int32_t *counts /*[C*H*W]*/, eg_stream_t stream);
int eg_indices_write(int32_t C, int32_t N, const float *means2d, const float *conics, const float *opacities,
                     const float *transmittances /*[C,H,W]*/, const int32_t *offsets /*[C,T+1]*/,
                     const int32_t *flatten_ids, int64_t n_isects, int32_t width, int32_t height, int32_t tile_size,
                     int32_t range_start, int32_t range_end, const int64_t *starts /*[C*H*W]*/, int64_t total,
                     int64_t *gaussian_ids, int64_t *pixel_ids, int64_t *camera_ids, eg_stream_t stream);
int eg_accumulate_fwd(const float *alpha /*[M]*/, const float *feat, int32_t feat_stride, int32_t channels,
                      const int64_t *starts /*[P]*/, const int64_t *counts /*[P]*/, int64_t P, int64_t M, float *render,
                      int32_t pixel_stride, float *alphas /*[P] or NULL*/, float *T_k /*[M] or NULL*/,
                      eg_stream_t stream);
int eg_accumulate_bwd(const float *alpha /*[M]*/, const float *feat, int32_t feat_stride, int32_t channels,
                      const int64_t *starts /*[P]*/, const int64_t *counts /*[P]*/, int64_t P, int64_t M,
                      const float *T_k /*[M]*/, const float *v_render, int32_t pixel_stride,
                      const float *v_alphas /*[P] or NULL*/, float *v_alpha /*[M]*/, int32_t add, float *v_feat,
                      eg_stream_t stream);

/* ---- gsplat's densification strategies (csrc/strategy.hip; edgegaussians_amd/strategy, edgegaussians_amd/relocation.py).
 * One lane per Gaussian, no atomics: the same bits every run.  Sizes are checked first (EG_ERR_ARG), an empty call is
 * EG_OK without a launch, then null pointers are refused by name.
 * eg_compute_relocation: gsplat `compute_relocation`.  r = clamp(ratios, 1, n_max), x = 1 - (1 - o)^(1/r),
 *   den = sum_{i=1..r} sum_{k=0..i-1} binoms[i-1, k] (-1)^k x^(k+1) / sqrt(k+1) in fp32 in that order;
 *   new_opacities = x, new_scales = (o / den) scales.  binoms is the row-major [n_max, n_max] table.
 * eg_inject_noise: means += R diag(s^2) R^T (noise * gate * scaler), s = exp(log_scales), R from the normalised quats
 *   (w, x, y, z), gate = 1 / (1 + exp(-100 ((1 - sigmoid(logit_opacities)) - 0.995))).  All [N, k] fp32.
 * eg_strategy_update / eg_strategy_update_packed: DefaultStrategy's running statistics over the visible pairs
 *   (radii > 0): grad2d[n] += |(gx width/2 C, gy height/2 C)|, count[n] += 1, radii_state[n] (or NULL) =
 *   max(radii_state[n], radii / max(width, height)), cameras in ascending order.  Dense: grads [C,N,2], radii [C,N].
 *   Packed: grads [nnz,2], radii [nnz], gaussian_ids [nnz], indptr [C+1] (unused and may be NULL when C == 1) over pairs
 *   in camera * N + gaussian order -- NOT checked: any other order gives wrong sums, never an access outside the
 *   tensors (segment bounds are clamped to [0, nnz], ids outside [0, N) match no lane). */
int eg_compute_relocation(const float *opacities /*[N]*/, const float *scales /*[N,3]*/, const int32_t *ratios /*[N]*/,
                          const float *binoms /*[n_max,n_max]*/, int32_t N, int32_t n_max, float *new_opacities /*[N]*/,
                          float *new_scales /*[N,3]*/, eg_stream_t stream);
int eg_inject_noise(float *means /*[N,3] in/out*/, const float *quats /*[N,4]*/, const float *log_scales /*[N,3]*/,
                    const float *logit_opacities /*[N]*/, const float *noise /*[N,3]*/, float scaler, int32_t N,
                    eg_stream_t stream);
int eg_strategy_update(const float *grads, const int32_t *radii, int32_t C, int32_t N, int32_t width, int32_t height,
                       float *grad2d /*[N]*/, float *count /*[N]*/, float *radii_state /*[N] or NULL*/,
                       eg_stream_t stream);
int eg_strategy_update_packed(const float *grads, const int32_t *radii, const int64_t *gaussian_ids,
                              const int64_t *indptr, int64_t nnz, int32_t C, int32_t N, int32_t width, int32_t height,
                              float *grad2d, float *count, float *radii_state, eg_stream_t stream);

/* ---- measurement aid: between eg_timing_begin(n) and eg_timing_end(), the next n eg_train_step
 * calls record HIP events between their stages on the launch stream; eg_timing_end synchronises
 * once and returns the average microseconds per stage (eg_timing_stage_count() entries, names by
 * eg_timing_stage_name(i)).  Not thread safe; one window at a time. */
int eg_timing_begin(int32_t n_steps);
/* tracing aid: eg_roctx_enable(1) dlopen's the ROCTx library and makes eg_train_step wrap its stages in
 * roctx ranges (eg:project_bin, eg:tile_sort, eg:composite_fwd, eg:footprint_bwd, eg:project_bwd_adam) -- rocprofv3
 * --marker-trace shows them next to the kernel trace; eg_roctx_enable(0) turns them off again (the default). */
int eg_roctx_enable(int32_t on);
/* debugging aid (process started with EG_FWD_PROF=1: the wave-autonomous forward runs its timed instantiation): the
 * per-wave phase records of the LAST forward launch, [items][4 quadrants][8] 64-bit words of shader-clock ticks (head,
 * staging, walk, publish, look-back, exact stop, epilogue; word 7 = 1 marks a wave that ran).  Returns the number of
 * 8-word records copied to the HOST buffer `out_host` (<= max_records) or a negative code.  Synchronises the device. */
int64_t eg_debug_fwd_profile(uint64_t *out_host, int64_t max_records);
int eg_timing_end(float *stage_us_host, int32_t *n_steps_out_host);
int eg_timing_stage_count(void);
const char *eg_timing_stage_name(int32_t i);

#ifdef __cplusplus
}
#endif
#endif /* EDGEGS_H */
