// Device code of the footprint backward (G8, order-independent form: DESIGN.md section 5) shared by composite.hip
// (footprint_bwd_kernel) and backward_fused.hip: the walk (moved out of composite.hip in round 6, unchanged) and the
// home phase around it (one copy since the lanes are dealt once per workgroup).  The derivation and the description of
// the walk sit in front of footprint_bwd_kernel in composite.hip.
#pragma once
#include "composite.h"
#include "deal_rule.h"

namespace eg {

struct Walk {
  int i0, fh;     // rows i0 .. i0 + fh - 1
  int pw;         // cells per row
  int jlo, jhi;   // inclusive column clip: gsplat's tile box, the image, the ellipse's extent
  int cells;      // fh * pw, 0 for an invisible Gaussian
  float thr;      // sigma threshold ln(255 o) (+ margin)
  float xoff, shear;  // first column of row i: ceil(xoff + shear * (y_g - (i + 0.5)))
};

__device__ __forceinline__ Walk walk_of(const float4 s0, const float4 s1, int width, int height) {
  Walk w;
  w.i0 = w.fh = w.pw = w.jlo = w.cells = 0;
  w.jhi = -1;
  w.thr = w.xoff = w.shear = 0.f;
  const int radius = __float_as_int(s1.w);
  // (the raw v_log_f32: 255 o >= 1 wherever the result is used, no denormal scaling needed; 1 ulp, inside the margin)
  const float thr = 0.693147180559945f * __builtin_amdgcn_logf(255.f * s1.y) + kThrMargin;
  const float det = s0.z * s1.x - s0.w * s0.w;
  if (radius <= 0 || !(thr > 0.f) || !(det > 0.f) || !(s0.z > 0.f)) return w;
  const int tw = (width + kTile - 1) / kTile, th = (height + kTile - 1) / kTile;
  int x0, y0, x1, y1;
  tile_box(s0.x, s0.y, radius, tw, th, x0, y0, x1, y1);  // pixels outside gsplat's box never see it
  // hardware sqrt / rcp (1 ulp): the 0.1 % + 0.01 px inflation swallows their error
  const float k = 2.f * thr * __builtin_amdgcn_rcpf(det);
  const float ex = __builtin_amdgcn_sqrtf(k * s1.x) * 1.001f + 0.01f;
  const float ey = __builtin_amdgcn_sqrtf(k * s0.z) * 1.001f + 0.01f;
  const int j0 = max(x0 * kTile, (int)ceilf(s0.x - ex - 0.5f));
  const int j1 = min(min(x1 * kTile, width) - 1, (int)floorf(s0.x + ex - 0.5f));
  const int i0 = max(y0 * kTile, (int)ceilf(s0.y - ey - 0.5f));
  const int i1 = min(min(y1 * kTile, height) - 1, (int)floorf(s0.y + ey - 0.5f));
  const int fw = j1 - j0 + 1, fh = i1 - i0 + 1;
  if (fw <= 0 || fh <= 0) return w;
  const float inv_a = __builtin_amdgcn_rcpf(s0.z);
  const float hw = __builtin_amdgcn_sqrtf(2.f * thr * inv_a) * 1.001f + 0.01f;
  const int pw = (int)(2.f * hw) + 1;
  w.i0 = i0; w.fh = fh; w.jlo = j0; w.jhi = j1; w.thr = thr;
  if (pw < fw) {
    w.pw = pw; w.shear = s0.w * inv_a; w.xoff = s0.x - hw - 0.5f;
  } else {
    w.pw = fw; w.shear = 0.f; w.xoff = (float)j0;
  }
  w.cells = w.pw * fh;
  return w;
}

struct Moments {
  float w_x, w_y, w_xx, w_xy, w_yy, abs_x, abs_y, v_o;
};

// One PAIR of horizontally adjacent cells of a footprint as the walk carries it from the prefetch to the visit: the two
// pixels' records (all zeros: nothing to visit) and the offset of the Gaussian's centre from the LEFT pixel's (the right
// pixel's is one less in x).
constexpr unsigned kOutOfImage = 0x80000000u;  // a byte offset no gtstop image reaches (launch_footprint_bwd checks)
typedef unsigned u32x3 __attribute__((ext_vector_type(3)));
struct Pair {
  u32x3 rec0, rec1;  // {gT bits, stop id, stop depth bits}: the pixel's last contributor, all ones if its walk did not stop
  float dx, dy;
};

// The quadratic form of a Gaussian as a visit uses it (round 5): sigma log2(e) = dx hx + dy hy with the HALF gradients
// hx = A dx + B dy, hy = B dx + C dy -- six operations give sigma and both components of d sigma / d (dx, dy), which the
// absgrad sums need anyway (|dL/dmean2d| of one pixel = |w| |a dx + b dy|, |w| |b dx + c dy|): the accepted part of a
// visit no longer forms a wx + b wy, b wx + c wy (six operations, now two), the exponential takes sigma log2(e) as it
// is, and the sums of |w| |h| are scaled by 2 / log2(e) once per lane.  One step to the right (dx - 1) takes A off hx
// and B off hy: the pair's second cell costs four operations.
struct Quad {
  float A, B, C;  // log2(e) / 2 * (a, b, c)
  float thr2;     // log2(e) * sigma threshold (> 0)
  float o;        // opacity
  bool high_o;    // (wave-uniform) some lane of the wave walks a Gaussian of opacity > 0.999
};
constexpr float kLog2e = 1.44269504088896341f;

__device__ __forceinline__ void footprint_cell(const Quad qd, unsigned g, unsigned dg, const u32x3 rec, float s2, float hx,
                                               float hy, float dx, float dy, Moments &m) {
  // One branch on the whole acceptance test (whole waves fall outside on large footprints, and on the steps whose
  // weight map is sparse), none after it: the lanes of a wave sit in up to eight footprints, accepted and rejected
  // pixels are mixed, and further branching only adds exec-mask bookkeeping.  The compares are what costs here (a
  // v_cmp takes the vector pipe ~1.5x as long as a multiply-add, tools/microbench): four of them --
  //   0 <= s2 <= thr2 as ONE unsigned compare of the bit patterns (a negative or NaN s2 has a pattern above any
  //   positive float's; s2 = -0 cannot arise: dx hx and dy hy would both have to be -0);
  //   where the walk of this pixel stopped only Gaussians at or before its last contributor count, (depth bits, id) <=
  //   (its depth bits, its id): "in front by depth" is one compare, the tie (the last contributor itself, or a twin at
  //   the very same depth) is looked at under a wave-uniform branch that is rarely taken.
  const float gT = __uint_as_float(rec.x);
  const bool in = __float_as_uint(s2) <= __float_as_uint(qd.thr2);
  bool counts = rec.z > dg;
  const bool tie = rec.z == dg;
  if (__builtin_amdgcn_ballot_w64(tie) != 0ull) {
    asm volatile("" ::: "memory");  // (a real branch: if-converted, the id compare would run on every visit)
    counts |= tie & (rec.y >= g);
  }
  if (!(gT != 0.f && in && counts)) return;
  const float vis = __builtin_amdgcn_exp2f(-s2);
  const float araw = qd.o * vis;
  // forward: skip if min(0.999, araw) < 1/255; gsplat's backward: no gradient through a clamped alpha (araw <= o:
  // only a wave that holds a Gaussian of opacity above 0.999 has to look)
  bool ok = araw >= kAlphaMin;
  if (qd.high_o) {
    asm volatile("" ::: "memory");
    ok &= araw <= kAlphaMax;
  }
  const float v_alpha = ok ? gT * __builtin_amdgcn_rcpf(1.f - araw) : 0.f;
  m.v_o += vis * v_alpha;
  const float w = -araw * v_alpha;
  const float wx = w * dx, wy = w * dy;
  m.w_x += wx; m.w_y += wy;
  m.w_xx += wx * dx; m.w_xy += wx * dy; m.w_yy += wy * dy;
  m.abs_x = fmaf(fabsf(w), fabsf(hx), m.abs_x);
  m.abs_y = fmaf(fabsf(w), fabsf(hy), m.abs_y);
}

__device__ __forceinline__ void footprint_visit(const Quad qd, unsigned g, unsigned dg, const Pair c, Moments &m) {
  const float dx = c.dx, dy = c.dy;
  const float hx = fmaf(qd.A, dx, qd.B * dy);
  const float hy = fmaf(qd.C, dy, qd.B * dx);
  const float s2 = fmaf(dx, hx, dy * hy);  // sigma log2(e)
  const float dx1 = dx - 1.f, hx1 = hx - qd.A, hy1 = hy - qd.B;
  const float s21 = fmaf(dx1, hx1, dy * hy1);
  footprint_cell(qd, g, dg, c.rec0, s2, hx, hy, dx, dy, m);
  footprint_cell(qd, g, dg, c.rec1, s21, hx1, hy1, dx1, dy, m);
}

// Lane r of n walks the PAIRS r, r + n, r + 2n, ... of Gaussian g's sheared box (its rows are cut into
// ceil(pw / 2) pairs of neighbouring cells; the odd cell out of an odd row's last pair lies outside the box, hence
// outside the ellipse: its own sigma test rejects it).  What a visit has to know about where it is -- row, first column
// of the row, the clip, the byte offset -- is worked out once per pair (round 5: it was once per cell, and together with
// the compares of the accept test it, not the accepted part, was where this kernel's time went: with the accepted part
// compiled out the launch at 1600 x 1200 took 152 of 174 us, with the loads compiled out as well 146); the two
// records of a pair are 24 contiguous bytes.  The records of the NEXT pair are prefetched while this one is evaluated;
// the loop body is written out twice with the two register sets swapping roles (a rotating copy cost ten moves per pair
// of visits), and the prefetch is unconditional: a cell with nothing to visit asks for an offset beyond the image.
__device__ __forceinline__ void footprint_walk(const float4 s0, const float4 s1, int g, int r, int n, int i0, int fh,
                                               int pw, int jlo, int jhi, float thr, float xoff,
                                               float shear, int width, const __amdgpu_buffer_rsrc_t gtstop, Moments &m) {
  const int ppr = (pw + 1) >> 1;  // pairs per row
  const float inv_ppr = __builtin_amdgcn_rcpf((float)ppr);
  // pair -> (row, pair in the row); the quotient estimate is exact for pairs < 2^21, the fix-up is free
  auto divmod = [&](int q, int &qi, int &qj) {
    qi = (int)(((float)q + 0.5f) * inv_ppr);
    qj = q - __mul24(qi, ppr);
    if (qj < 0) { qj += ppr; --qi; }
    if (qj >= ppr) { qj -= ppr; ++qi; }
  };
  const int width12 = width * (int)sizeof(StopRec);
  // (centre - 0.5 once per Gaussian: the pixel centres are at integer + 0.5)
  const float xc = s0.x - 0.5f, yc = s0.y - 0.5f;
  // The records come through buffer loads: a 32-bit byte offset on the uniform descriptor (two full-rate 24-bit
  // multiply-adds and the load's own address adder instead of a quarter-rate 64-bit multiply-add per visit), and a
  // cell with nothing to visit -- past the lane's last pair or outside the column clip -- asks for an offset beyond the
  // image: the hardware's range check returns zeros without touching memory, and gT == 0 is "skip".  "Nothing to
  // visit" is the sign bit of (j - jlo) | (jhi - j) | (pairs left - 1), moved into the offset's top bit: no compare.
  auto fetch = [&](int i, int cp, int live1) -> Pair {
    Pair p;
    p.dy = yc - (float)i;
    const int j = (int)ceilf(xoff + shear * p.dy) + 2 * cp;
    const int t1 = j - jlo, t2 = jhi - j;
    const unsigned bad0 = (unsigned)(t1 | t2 | live1) & kOutOfImage;
    const unsigned bad1 = (unsigned)((t1 + 1) | (t2 - 1) | live1) & kOutOfImage;
    const unsigned base = (unsigned)(__mul24(i, width12) + __mul24(j, 12));
    p.rec0 = __builtin_amdgcn_raw_buffer_load_b96(gtstop, (int)(bad0 | base), 0, 0);
    p.rec1 = __builtin_amdgcn_raw_buffer_load_b96(gtstop, (int)(bad1 | (base + 12u)), 0, 0);
    p.dx = xc - (float)j;
    return p;
  };
  const unsigned ug = (unsigned)g, dg = (unsigned)__float_as_int(s1.z);
  const Quad qd = {0.5f * kLog2e * s0.z, 0.5f * kLog2e * s0.w, 0.5f * kLog2e * s1.x, kLog2e * thr, s1.y,
                   __builtin_amdgcn_ballot_w64(s1.y > kAlphaMax) != 0ull};
  int di, dc;
  divmod(n, di, dc);
  int ia, ca;
  divmod(r, ia, ca);
  ia += i0;
  int left = __mul24(fh, ppr) - r;  // > 0 while the lane still has a pair
  auto advance = [&]() {
    left -= n;
    // (the carry without a compare: t = c + dc - ppr, its sign mask is -1 for "no carry")
    const int t = ca + dc - ppr, sm = t >> 31;
    ca = t + (ppr & sm);
    ia += di + 1 + sm;
  };
  Pair p0 = fetch(ia, ca, left - 1);
  while (left > 0) {
    advance();
    const Pair p1 = fetch(ia, ca, left - 1);
    footprint_visit(qd, ug, dg, p0, m);
    if (left <= 0) break;
    advance();
    p0 = fetch(ia, ca, left - 1);
    footprint_visit(qd, ug, dg, p1, m);
  }
}

// ---------------------------------------------------------------------------------------------
// The home phase: what a wave does around the walk.  Everything in it that is a function of the workgroup's Gaussians
// alone -- the sizes of the footprints (round 5), how each wave's 64 lanes are dealt to its 8 Gaussians, the Gaussians'
// splat records -- is worked out ONCE, by the sizing lanes (one Gaussian per lane of the workgroup's first wave) in front
// of the workgroup's barrier, and handed to the waves through LDS:
//   the Gaussian's row of s_walk, 12 words:  i0 fh pw jlo | jhi cells thr xoff | shear - n first
//   the wave's INBOX, 72 words at the front of the wave's slice of the partial-record exchange (which the wave
//   overwrites only after its walk):  8 x {s0, s1} | total first[1] .. first[7]
// Behind the barrier a lane finds its Gaussian k with seven compares against the broadcast firsts, takes n, first, the
// walk and the record from row / inbox entry k, and walks.  (Before, every wave dealt its own lanes -- two three-round
// shuffle butterflies, a three-round shuffle scan, seven readlanes, three more shuffles -- and every lane gathered its
// Gaussian's record from global memory a second time, behind the barrier and the dealing.)
constexpr int kHomeRow = 12;     // words of a Gaussian's s_walk row
constexpr int kHomeInbox = 72;   // words of a wave's inbox
constexpr int kHomeFoldPad = 3;  // partial records footprint_fold may read (and discard) behind a wave's last one

// Sizing lane t (of the workgroup's first wave; the lanes t & ~7 .. t | 7 take part together) and Gaussian hg: `row` is
// hg's s_walk row, `rows8` the row of the first Gaussian of hg's wave, `inbox` that wave's inbox.
__device__ __forceinline__ void footprint_size_and_deal(const float4 *__restrict__ splat, int hg, int N, int width,
                                                        int height, int t, int *row, const int *rows8, float *inbox) {
  // (a Gaussian behind the last one has no footprint; its inbox entry is the LAST Gaussian's record, which is what the
  // idle lanes of a ragged wave walk with: footprint_home_walk clamps g the same way)
  const int gc = min(hg, N - 1);
  const float4 s0 = splat[2 * gc], s1 = splat[2 * gc + 1];
  Walk w = walk_of(make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), width, height);
  if (hg < N) w = walk_of(s0, s1, width, height);
  int4 *dst = (int4 *)row;
  dst[0] = make_int4(w.i0, w.fh, w.pw, w.jlo);
  dst[1] = make_int4(w.jhi, w.cells, __float_as_int(w.thr), __float_as_int(w.xoff));
  const int i = t & 7;
  *(float4 *)(inbox + 8 * i) = s0;
  *(float4 *)(inbox + 8 * i + 4) = s1;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  int cells[kDealGroups];
#pragma unroll
  for (int j = 0; j < kDealGroups; ++j) cells[j] = rows8[kHomeRow * j + 5];
  int total, live;
  deal_totals(cells, total, live);
  Deal d = {0, 0};
  if (total > 0) d = deal_lanes(cells, live, __builtin_amdgcn_rcpf((float)total), i);
  dst[2] = make_int4(__float_as_int(w.shear), 0, d.n, d.first);
  inbox[64 + i] = __int_as_float(i == 0 ? total : d.first);  // (first[0] is 0 whatever the wave holds)
}

// A wave behind the barrier: lane -> (Gaussian k, lane r of n), the walk.  rows8: the s_walk row of the wave's first
// Gaussian, gbase.  s0, s1 come back for the caller's partial record (zeros if the wave holds no footprint at all).
__device__ __forceinline__ void footprint_home_walk(const int *rows8, const float *inbox, int lane, int gbase, int N,
                                                    int width, const __amdgpu_buffer_rsrc_t rec_rsrc, float4 &s0,
                                                    float4 &s1, Moments &m) {
  const float4 f0 = *(const float4 *)(inbox + 64), f1 = *(const float4 *)(inbox + 68);
  s0 = s1 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (__float_as_int(f0.x) <= 0) return;  // (total: wave-uniform)
  // lane -> Gaussian: the group whose lane range holds this lane (a lane past the last range idles)
  const int k = (lane >= __float_as_int(f0.y)) + (lane >= __float_as_int(f0.z)) + (lane >= __float_as_int(f0.w)) +
                (lane >= __float_as_int(f1.x)) + (lane >= __float_as_int(f1.y)) + (lane >= __float_as_int(f1.z)) +
                (lane >= __float_as_int(f1.w));
  const int4 *wk = (const int4 *)(rows8 + kHomeRow * k);
  const int4 a = wk[0], b = wk[1], c = wk[2];
  const int n = max(c.z, 1);
  const int r = lane - c.w;
  const int g = min(gbase + k, N - 1);
  const int cells = r < n ? b.y : 0;
  s0 = *(const float4 *)(inbox + 8 * k);
  s1 = *(const float4 *)(inbox + 8 * k + 4);
  footprint_walk(s0, s1, g, r, n, a.x, cells > 0 ? a.y : 0, max(a.z, 1), a.w, b.x, __int_as_float(b.z),
                 __int_as_float(b.w), __int_as_float(c.x), width, rec_rsrc, m);
}

// The first half of a lane's partial g2d record, vx vy |vx| |vy|, from its moments (the absgrad sums were taken over
// |w| |h|, h = log2(e) / 2 times the gradient of sigma: footprint_visit).  vx = a w_x + b w_y and vy = b w_x + c w_y are
// a product and a multiply-add each, and WHICH product is the rounded one is written out: left to the compiler's
// contraction of a * b + c * d it changed with the code around the expression, and with it the last bits of every
// gradient.  (These are the forms the kernels were compiled to while they carried the expression themselves.)
__device__ __forceinline__ float4 footprint_partial_means(const float4 s0, const float4 s1, const Moments &m) {
  return make_float4(fmaf(s0.z, m.w_x, s0.w * m.w_y), fmaf(s1.x, m.w_y, s0.w * m.w_x), (2.f / kLog2e) * m.abs_x,
                     (2.f / kLog2e) * m.abs_y);
}

// Lane (k, component) adds component `p[0]` of the partial records of Gaussian k's n lanes in lane order: a left fold,
// p[0] + p[STRIDE] + ...  Four records are requested together in front of the dependent adds (one read, one wait, one
// add and one branch per record before); a read behind the n-th record is discarded -- the running sum is never -0, so
// adding +0 leaves its bits alone -- and may reach kHomeFoldPad records behind the wave's last one.
template <int STRIDE>
__device__ __forceinline__ float footprint_fold(const float *p, int n) {
  float sum = 0.f;
  for (int t = 0; t < n; t += 4, p += 4 * STRIDE) {
    const float v0 = p[0], v1 = p[STRIDE], v2 = p[2 * STRIDE], v3 = p[3 * STRIDE];
    sum += v0;
    sum += t + 1 < n ? v1 : 0.f;
    sum += t + 2 < n ? v2 : 0.f;
    sum += t + 3 < n ? v3 : 0.f;
  }
  return sum;
}

}  // namespace eg
