// Stand-alone host check of the per-drone arithmetic in csrc/planner_sizes.h,
// csrc/cem_sizes.h and csrc/step_score.h (no GPU, no HIP): the byte sizes of a
// per-drone planner's buffers and of ret_agent with their overflow refusals, the
// shape the update / refit kernels run over, the variant chosen from it and the
// launch grids.  Built and run by tests/test_per_drone_host.py with
// -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>

#include "cem_sizes.h"
#include "planner_sizes.h"
#include "step_score.h"

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  using namespace qs;
  const uint64_t lim = uint64_t(1) << 31;
  uint64_t b[kMppiBufs], e[kMppiBufs], ra = 0;

  // ---- MPPI: the flagship shape; only weights and best differ from the env-level sizes
  const MppiShape c3{16, 4096, 1, 8, 1};
  CHECK(mppi_sizes(c3, e) && mppi_pd_sizes(c3, b, &ra));
  CHECK(ra == 4096u * 8 * 8 && b[kMppiWeights] == ra && b[kMppiBest] == 8u * 4);
  CHECK(e[kMppiWeights] == 4096u * 8 && e[kMppiBest] == 4u);
  for (int i = 0; i < kMppiBufs; ++i)
    if (i != kMppiWeights && i != kMppiBest) CHECK(b[i] == e[i]);
  // odd sizes, A = 4
  const MppiShape a4{7, 3, 21, 3, 4};
  CHECK(mppi_pd_sizes(a4, b, &ra) && ra == 3u * 21 * 3 * 8 && b[kMppiBest] == 21u * 3 * 4);
  CHECK(b[kMppiCandidates] == 7u * 3 * 21 * 3 * 4 * 4 && b[kMppiRet] == 3u * 21 * 8 && b[kMppiFirstDone] == 3u * 21 * 4);

  // whatever mppi_sizes refuses is refused, and ra is not needed for that
  CHECK(!mppi_pd_sizes(MppiShape{0, 4, 1, 8, 1}, b, &ra) && !mppi_pd_sizes(MppiShape{33, 4, 1, 8, 1}, b, &ra));
  CHECK(!mppi_pd_sizes(MppiShape{8, 1, 1, 8, 1}, b, &ra) && !mppi_pd_sizes(MppiShape{8, 4, 1, 65, 4}, b, &ra));
  CHECK(!mppi_pd_sizes(MppiShape{8, 4, 1, 8, 5}, b, &ra) && !mppi_pd_sizes(MppiShape{8, 4, 0, 8, 1}, b, &ra));
  CHECK(!mppi_pd_sizes(MppiShape{8, -4, 1, 8, 1}, b, &ra));

  // ret_agent: C · E · D · 8 bytes below 2^31, i.e. C · E · D < 2^28
  CHECK(mppi_sizes(MppiShape{8, 1 << 12, 1 << 12, 16, 1}, e));                 // 2^28 agents: the env-level planner takes it
  CHECK(!mppi_pd_sizes(MppiShape{8, 1 << 12, 1 << 12, 16, 1}, b, &ra));        // ... ret_agent would be 2^31 bytes
  CHECK(mppi_pd_sizes(MppiShape{8, 1 << 12, 1 << 12, 15, 1}, b, &ra) && ra == (uint64_t(15) << 27) && ra < lim);
  CHECK(mppi_pd_sizes(MppiShape{8, (1 << 12) - 1, 1 << 12, 16, 1}, b, &ra) && ra == (uint64_t((1 << 12) - 1) << 19));
  CHECK(!mppi_pd_sizes(MppiShape{8, 1 << 26, 1, 4, 1}, b, &ra) && mppi_pd_sizes(MppiShape{8, 1 << 26, 1, 3, 1}, b, &ra));
  // products past 32 bits and past 64 bits: refused before anything is narrowed
  CHECK(!mppi_pd_sizes(MppiShape{8, 1 << 16, 1 << 16, 1, 1}, b, &ra));         // C · E = 2^32
  CHECK(!mppi_pd_sizes(MppiShape{8, 1 << 20, 1 << 20, 64, 1}, b, &ra));        // C · E · D = 2^46
  CHECK(!mppi_pd_sizes(MppiShape{8, 4, int64_t(1) << 31, 1, 1}, b, &ra));
  CHECK(!mppi_pd_sizes(MppiShape{8, 4, int64_t(1) << 40, int64_t(1) << 40, 1}, b, &ra));   // E · D = 2^80
  CHECK(!mppi_pd_sizes(MppiShape{8, 4, int64_t(1) << 62, 4, 1}, b, &ra));                  // E · D wraps to 0 in 64 bits
  CHECK(!mppi_pd_sizes(MppiShape{8, int64_t(1) << 33, int64_t(1) << 33, 1, 1}, b, &ra));   // C · E = 2^66
  // the workgroup-per-(agent, step) grid: n · E · D below 2^31
  CHECK(mppi_pd_sizes(MppiShape{31, 2, 1 << 21, 32, 1}, b, &ra) && ra == (uint64_t(1) << 30));   // 31 · 2^26 < 2^31
  CHECK(!mppi_pd_sizes(MppiShape{32, 2, 1 << 21, 32, 1}, b, &ra));             // 32 · 2^26 = 2^31 (ret_agent itself fits)
  CHECK(mppi_sizes(MppiShape{32, 2, 1 << 21, 32, 1}, e));

  // ---- the shape the update runs over, its variant and grids
  {
    const MppiShape u = mppi_pd_shape(c3);
    CHECK(u.n == 16 && u.C == 4096 && u.E == 8 && u.D == 1 && u.A == 1);
    CHECK(mppi_variant(u.E, u.C, u.D * u.A) == kMppiPerBlock);
    const MppiGrids g = mppi_grids(u, kMppiPerBlock), ge = mppi_grids(c3, kMppiPerBlock);
    CHECK(g.sample == ge.sample && g.sample == 4096u * 8 / 256);                // one thread per (c, e, d) either way
    CHECK(g.weights == 8u && g.sum == 8u * 16 && ge.weights == 1u && ge.sum == 16u);
  }
  {
    const MppiShape s{7, 3, 300, 3, 4}, u = mppi_pd_shape(s);
    CHECK(u.E == 900 && u.D == 1 && u.A == 4 && mppi_variant(u.E, u.C, u.A) == kMppiPerThread);
    const MppiGrids g = mppi_grids(u, kMppiPerThread), ge = mppi_grids(s, kMppiPerThread);
    CHECK(g.weights == 4u && ge.weights == 2u);                                 // 900 agents, 300 envs: 256 a workgroup
    CHECK(g.sum == ge.sum && g.sum == mppi_div_up(7u * 300 * 3 * 4, 256));      // one thread per (j, e, d, a) either way
    CHECK(g.sample == ge.sample);
  }
  // the variant's boundary moves with the units: E · D · A < 16 384 elements in both modes, C >= 64
  CHECK(mppi_variant(2047 * 8, 64, 1) == kMppiPerBlock && mppi_variant(2048 * 8, 64, 1) == kMppiPerThread);
  CHECK(mppi_variant(2047 * 8, 63, 1) == kMppiPerThread);
  CHECK(mppi_row_pow2(1) == 1 && mppi_row_pow2(3) == 4 && mppi_row_pow2(4) == 4);   // a drone's row

  // ---- CEM
  uint64_t cb[kCemBufs], ce[kCemBufs];
  const CemShape k3{16, 4096, 512, 3, 1, 8, 1};
  CHECK(cem_sizes(k3, ce) && cem_pd_sizes(k3, cb, &ra) && ra == 4096u * 8 * 8);
  CHECK(cb[kCemElites] == 512u * 8 * 4 && cb[kCemIterBest] == 3u * 8 * 8 && ce[kCemElites] == 512u * 4 && ce[kCemIterBest] == 24u);
  for (int i = 0; i < kCemBufs; ++i)
    if (i != kCemElites && i != kCemIterBest) CHECK(cb[i] == ce[i]);
  CHECK(cem_pd_sizes(CemShape{7, 9, 3, 2, 21, 3, 4}, cb, &ra) && cb[kCemElites] == 3u * 63 * 4 && cb[kCemIterBest] == 2u * 63 * 8);
  // K and I at their bounds with the most agents ret_agent allows: 64-bit products, nothing narrowed
  CHECK(cem_pd_sizes(CemShape{2, 1024, 1024, 16, 1 << 12, 63, 1}, cb, &ra));
  CHECK(cb[kCemElites] == uint64_t(1024) * 63 * 4096 * 4 && cb[kCemIterBest] == uint64_t(16) * 63 * 4096 * 8);
  CHECK(cb[kCemElites] < lim && ra == uint64_t(1024) * 4096 * 63 * 8 && ra < lim);
  CHECK(!cem_pd_sizes(CemShape{2, 1024, 1024, 16, 1 << 12, 64, 1}, cb, &ra));       // C · E · D = 2^28
  CHECK(cem_sizes(CemShape{2, 1024, 1024, 16, 1 << 12, 64, 1}, ce));
  // what cem_sizes refuses, and the overflowing products
  CHECK(!cem_pd_sizes(CemShape{8, 4, 5, 1, 1, 8, 1}, cb, &ra) && !cem_pd_sizes(CemShape{8, 4, 1, 17, 1, 8, 1}, cb, &ra));
  CHECK(!cem_pd_sizes(CemShape{8, 4, 0, 1, 1, 8, 1}, cb, &ra) && !cem_pd_sizes(CemShape{8, 4096, 1025, 1, 1, 8, 1}, cb, &ra));
  CHECK(!cem_pd_sizes(CemShape{8, 1 << 16, 8, 3, 1 << 16, 1, 1}, cb, &ra));
  CHECK(!cem_pd_sizes(CemShape{8, 4, 1, 1, int64_t(1) << 40, int64_t(1) << 40, 1}, cb, &ra));
  CHECK(!cem_pd_sizes(CemShape{8, 4, 1, 1, int64_t(1) << 62, 4, 1}, cb, &ra));
  {
    const CemShape u = cem_pd_shape(k3);
    CHECK(u.n == 16 && u.C == 4096 && u.K == 512 && u.I == 3 && u.E == 8 && u.D == 1 && u.A == 1);
    CHECK(cem_variant(u.E, u.C, u.D * u.A) == kCemPerBlock);
    const CemGrids g = cem_grids(u, kCemPerBlock), ge = cem_grids(k3, kCemPerBlock);
    CHECK(g.fill == ge.fill && g.sample == ge.sample && g.finish == ge.finish);   // these run over the same elements
    CHECK(g.select == 8u && g.refit == 8u * 16 && ge.select == 1u && ge.refit == 16u);
    const CemShape t{5, 9, 3, 2, 300, 3, 4}, ut = cem_pd_shape(t);
    CHECK(cem_variant(ut.E, ut.C, ut.A) == kCemPerThread);
    const CemGrids gt = cem_grids(ut, kCemPerThread), gte = cem_grids(t, kCemPerThread);
    CHECK(gt.select == 4u && gte.select == 2u && gt.refit == gte.refit && gt.fill == gte.fill);
    CHECK(cem_variant(1 << 20, 512, 1) == kCemPerBlock && cem_variant(1 << 20, 511, 1) == kCemPerThread);
  }

  // ---- qs_score_agents: ret_agent's bytes and its place among the ranges of a call
  {
    uint64_t sb[kScoreOuts], act = 0;
    const ScoreShape s{3, 21, 8, 27, 1, 4};
    CHECK(score_sizes(s, sb, &act) && score_agent_bytes(s) == 3u * 21 * 8 * 8 && score_fits(score_agent_bytes(s)));
    const ScoreShape big{1 << 12, 1 << 12, 16, 27, 1, 4};                     // 2^28 agents: the launch fits, ret_agent does not
    CHECK(score_sizes(big, sb, &act) && score_agent_bytes(big) == lim && !score_fits(score_agent_bytes(big)));
    const ScoreShape most{(1 << 28) - 1, 1, 1, 27, 1, 4};
    CHECK(score_sizes(most, sb, &act) && score_fits(score_agent_bytes(most)));
    const ScoreShape edge{2147483647, 1, 1, 27, 1, 4};                        // the most agents score_sizes takes: 2^34 - 8 bytes
    CHECK(score_sizes(edge, sb, &act) && score_agent_bytes(edge) == (uint64_t(1) << 34) - 8 && !score_fits(score_agent_bytes(edge)));
    // a full call names n · (7 outputs + 1 action buffer) + ret + first_done + ret_agent ranges
    CHECK(kScoreMaxRanges == kScoreMaxSteps * (kScoreStepOuts + 1) + 3);
    static char m[4096];
    ScoreRanges r;
    CHECK(r.add(m, 64, true) && r.add(m + 64, 8, false) && r.add(m + 72, 4, false) && r.add(m + 128, 3 * 8, false) && !r.overlap());
    ScoreRanges q;                                                             // ret_agent over an action buffer / over ret
    CHECK(q.add(m, 64, true) && q.add(m + 60, 24, false) && q.overlap());
    ScoreRanges w;
    CHECK(w.add(m + 64, 8, false) && w.add(m + 64, 24, false) && w.overlap());
  }
  std::printf("per_drone sizes ok\n");
  return 0;
}
