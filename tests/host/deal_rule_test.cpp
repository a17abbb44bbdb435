// Host test of the footprint backward's lane dealing (edgegaussians_amd/csrc/deal_rule.h): a stand-alone program.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I edgegaussians_amd/csrc
//       tests/host/deal_rule_test.cpp -o deal_rule_test && ./deal_rule_test
//
// (tests/test_footprint_home_host.py builds it without the sanitizers and runs it with the suite.)  Over adversarial
// mixes of eight cell counts -- all zero, one live, 1 beside 2^22, eight equal, random -- and with the reciprocal of the
// total exact, one ulp low and one ulp high (the device's v_rcp_f32 is 1 ulp off), it asserts:
//   every live footprint has at least one lane, a dead one none;
//   the lane ranges are contiguous, disjoint and increasing, the first one starting at lane 0;
//   the lanes sum to at most 64 -- and to exactly 64 whenever slack <= live, which the rule's arithmetic makes always.
// Exit status 0 and "ok" on success; the first violated invariant otherwise.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "deal_rule.h"

static int g_checked = 0;

static void fail(const char *what, const int (&cells)[8], float inv) {
  std::fprintf(stderr, "deal_rule_test: %s for cells {%d %d %d %d %d %d %d %d}, inv_total %a\n", what, cells[0], cells[1],
               cells[2], cells[3], cells[4], cells[5], cells[6], cells[7], inv);
  std::exit(1);
}

static void check(const int (&cells)[8]) {
  int total, live;
  eg::deal_totals(cells, total, live);
  int t = 0, l = 0;
  for (int j = 0; j < 8; ++j) { t += cells[j]; l += cells[j] > 0; }
  if (t != total || l != live) fail("deal_totals", cells, 0.f);
  if (total == 0) { ++g_checked; return; }  // (the kernel deals nothing: every n is 0)
  const float exact = 1.f / (float)total;
  const float invs[3] = {exact, std::nextafterf(exact, 0.f), std::nextafterf(exact, 1.f)};
  for (float inv : invs) {
    int next = 0, plain = 0;  // plain: the lanes before the slack is handed out
    eg::Deal d[8];
    for (int i = 0; i < 8; ++i) d[i] = eg::deal_lanes(cells, live, inv, i);
    for (int i = 0; i < 8; ++i) {
      if (cells[i] > 0 && d[i].n < 1) fail("a live footprint without a lane", cells, inv);
      if (cells[i] <= 0 && d[i].n != 0) fail("a dead footprint with lanes", cells, inv);
      if (d[i].first != next) fail("ranges not contiguous from lane 0", cells, inv);
      if (d[i].first < 0 || d[i].n < 0) fail("negative range", cells, inv);
      next = d[i].first + d[i].n;
    }
    if (next > eg::kDealLanes) fail("more than 64 lanes", cells, inv);
    // slack = 64 - (sum before the hand-out); the hand-out gives min(slack, live) lanes
    const float share = (float)(64 - live) * (1.f - 1e-5f) * inv;
    for (int j = 0; j < 8; ++j) plain += cells[j] > 0 ? 1 + (int)((float)cells[j] * share) : 0;
    const int slack = 64 - plain;
    if (slack < 0) fail("negative slack", cells, inv);
    if (slack > live) fail("slack above live (idle lanes)", cells, inv);
    if (next != eg::kDealLanes) fail("fewer than 64 lanes although slack <= live", cells, inv);
    ++g_checked;
  }
}

int main() {
  uint64_t s = 0x9e3779b97f4a7c15ull;
  auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  {
    const int zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    check(zero);
  }
  const int sizes[] = {1, 2, 3, 7, 50, 81, 4095, 1 << 16, 1 << 22, (1 << 22) + 1, 1 << 24, (1 << 27) - 1};
  for (int v : sizes) {
    for (int pos = 0; pos < 8; ++pos) {  // one live
      int c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      c[pos] = v;
      check(c);
      for (int q = 0; q < 8; ++q) {      // 1 (and 2^22) beside v
        if (q == pos) continue;
        int c2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        c2[pos] = v; c2[q] = 1;
        check(c2);
        int c3[8] = {1, 1, 1, 1, 1, 1, 1, 1};
        c3[pos] = v; c3[q] = 1 << 22;
        check(c3);
      }
    }
    const int eq[8] = {v, v, v, v, v, v, v, v};  // eight equal
    check(eq);
    for (int k = 1; k < 8; ++k) {                // k equal, the rest dead: in front, behind, alternating
      int a[8] = {0}, b[8] = {0}, c[8] = {0};
      for (int j = 0; j < k; ++j) { a[j] = v; b[7 - j] = v; c[(2 * j) % 8 + (2 * j) / 8] = v; }
      check(a); check(b); check(c);
    }
  }
  for (int it = 0; it < 200000; ++it) {  // random: log-uniform sizes, a random share dead (sums stay below 2^31)
    int c[8];
    const unsigned dead = (unsigned)(rnd() & 0xff) & (unsigned)(rnd() & 0xff);
    for (int j = 0; j < 8; ++j) {
      const int bits = (int)(rnd() % 27);
      c[j] = ((dead >> j) & 1u) ? 0 : 1 + (int)(rnd() & ((1u << bits) - 1u));
    }
    check(c);
  }
  std::printf("ok: %d deals checked\n", g_checked);
  return 0;
}
