// How a wavefront of the footprint backward hands its 64 lanes to its 8 Gaussians, as a plain
// function of the eight cell counts: one lane for every live footprint, the other 64 - live in proportion to the cell
// counts (rounded down), the slack one each to the first live groups.  No HIP in here: footprint_dev.h runs it on the
// sizing lanes, tests/host/deal_rule_test.cpp on the host under the sanitizers.
#pragma once

#if defined(__HIPCC__)
#define EG_DEAL_HD __host__ __device__ __forceinline__
#else
#define EG_DEAL_HD inline
#endif

namespace eg {

constexpr int kDealLanes = 64, kDealGroups = 8;

struct Deal {
  int n, first;  // group i's lanes are first .. first + n - 1 (n == 0: a footprint without cells)
};

EG_DEAL_HD void deal_totals(const int (&cells)[kDealGroups], int &total, int &live) {
  total = 0; live = 0;
  for (int j = 0; j < kDealGroups; ++j) {
    total += cells[j];
    live += cells[j] > 0 ? 1 : 0;
  }
}

// Group i's share.  total > 0, inv_total ~ 1 / total (the device's v_rcp_f32 is 1 ulp off: the factor 1 - 1e-5 keeps the
// sum of the rounded-down shares at or below 64 - live all the same).
EG_DEAL_HD Deal deal_lanes(const int (&cells)[kDealGroups], int live, float inv_total, int i) {
  const float share = (float)(kDealLanes - live) * (1.f - 1e-5f) * inv_total;
  int sum = 0, before = 0, rank = 0, mine = 0;  // rank: live groups before this one
  // (no cells[i]: a register array indexed by a run-time value would go to scratch memory on the device)
  for (int j = 0; j < kDealGroups; ++j) {
    const int nj = cells[j] > 0 ? 1 + (int)((float)cells[j] * share) : 0;
    if (j < i) { before += nj; rank += cells[j] > 0 ? 1 : 0; }
    if (j == i) mine = nj;
    sum += nj;
  }
  const int slack = kDealLanes - sum;
  Deal d;
  d.first = before + (rank < slack ? rank : slack);
  d.n = mine + ((mine > 0 && rank < slack) ? 1 : 0);
  return d;
}

}  // namespace eg
