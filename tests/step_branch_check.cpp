// Stand-alone host check of csrc/step_branch.h (no GPU, no HIP): the sizes of a
// branch set's blocks at the 2^31 edges, how a rollout of any length is cut into
// launches, and the live / first-done rule of the accumulators over chains
// against a straight loop.
// Built and run by tests/test_step_branch_host.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "step_branch.h"

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

// ret / first_done of `total` steps in one go: the rule's plain statement
static qs::BranchAcc straight(const std::vector<double>& rew, const std::vector<uint8_t>& done) {
  qs::BranchAcc a;
  const int total = (int)rew.size();
  a.first_done = total;
  for (int j = 0; j < total; ++j) {
    a.ret += rew[j];
    if (done[j]) {
      a.first_done = j;
      break;
    }
  }
  return a;
}

int main() {
  using qs::BranchShape;
  using qs::BranchSizes;
  const uint64_t lim = uint64_t(1) << 31;
  BranchSizes z;
  // ---- sizes.  C = 3 candidates of 21 envs × 8 drones, 29 fp32 fields, 15 slots of 1 float
  std::memset(&z, 0, sizeof(z));
  CHECK(qs::branch_sizes(BranchShape{3, 21, 8, 15, 1, 29, 4}, &z));
  CHECK(z.V == 63 && z.N == 504);
  CHECK(z.bytes[0] == 504u * 29 * 4 && z.bytes[1] == 63u * 32 && z.bytes[2] == 15u * 504 * 4);
  CHECK(z.bytes[3] == 63u * 8 && z.bytes[4] == 63u * 4 && z.bytes[5] == 504u * 8);
  uint64_t end = 0;
  for (int i = 0; i < qs::kBranchBlocks; ++i) {   // blocks in order, aligned, not overlapping
    CHECK(z.offset[i] % qs::kBranchAlign == 0 && z.offset[i] >= end);
    end = z.offset[i] + z.bytes[i];
  }
  CHECK(z.total >= end && z.total % qs::kBranchAlign == 0);
  // fp64, A = 4
  CHECK(qs::branch_sizes(BranchShape{2, 5, 8, 15, 4, 29, 8}, &z) && z.bytes[0] == 80u * 29 * 8 && z.bytes[2] == 15u * 80 * 16);
  // bad shapes
  CHECK(!qs::branch_sizes(BranchShape{0, 21, 8, 15, 1, 29, 4}, &z));
  CHECK(!qs::branch_sizes(BranchShape{-1, 21, 8, 15, 1, 29, 4}, &z));
  CHECK(!qs::branch_sizes(BranchShape{3, 21, 8, 0, 1, 29, 4}, &z));
  CHECK(!qs::branch_sizes(BranchShape{3, 21, 8, 15, 1, 29, 0}, &z));
  // the agent block at 2^31 bytes: N · 32 fields · 4 bytes, N = 2^24 is 2^31 exactly; one env less fits
  CHECK(!qs::branch_sizes(BranchShape{1 << 12, 1 << 9, 8, 1, 1, 32, 4}, &z));
  CHECK(qs::branch_sizes(BranchShape{(1 << 12), (1 << 9) - 1, 8, 1, 1, 32, 4}, &z) && z.bytes[0] < lim);
  CHECK(z.bytes[0] == (uint64_t)(1 << 12) * ((1 << 9) - 1) * 8 * 128);
  // the history block at 2^31 bytes: N · H · A · 4 with N = 2^20, H · A = 512
  CHECK(!qs::branch_sizes(BranchShape{1 << 10, 1 << 7, 8, 128, 4, 1, 4}, &z));
  CHECK(qs::branch_sizes(BranchShape{1 << 10, 1 << 7, 8, 127, 4, 1, 4}, &z) && z.bytes[2] < lim);
  // ret_agent at 2^31 bytes: N = 2^28 doubles
  CHECK(!qs::branch_sizes(BranchShape{1 << 13, 1 << 12, 8, 1, 1, 1, 4}, &z));
  CHECK(qs::branch_sizes(BranchShape{(1 << 13) - 1, 1 << 12, 8, 1, 1, 1, 4}, &z) && z.bytes[5] < lim);
  // the env records at 2^31 bytes: V = 2^26 records of 32 bytes (D = 1, so N = V)
  CHECK(!qs::branch_sizes(BranchShape{1 << 13, 1 << 13, 1, 1, 1, 1, 4}, &z));
  CHECK(qs::branch_sizes(BranchShape{(1 << 13) - 1, 1 << 13, 1, 1, 1, 1, 4}, &z) && z.bytes[1] < lim);
  // V and N at 2^31 and far past it: refused without wrapping
  CHECK(!qs::branch_sizes(BranchShape{1 << 16, 1 << 15, 1, 1, 1, 1, 1}, &z));
  CHECK(!qs::branch_sizes(BranchShape{1 << 15, 1 << 15, 2, 1, 1, 1, 1}, &z));
  CHECK(!qs::branch_sizes(BranchShape{INT32_MAX, INT32_MAX, 64, 1, 1, 1, 1}, &z));
  CHECK(!qs::branch_sizes(BranchShape{INT64_MAX, 2, 2, 1, 1, 1, 1}, &z));
  CHECK(!qs::branch_sizes(BranchShape{2, 2, 2, INT64_MAX, INT64_MAX, 1, 1}, &z));
  CHECK(!qs::branch_sizes(BranchShape{2, 2, 2, 1, 1, INT64_MAX, INT64_MAX}, &z));

  // ---- cutting: lengths 1, depth, depth + 1 and 3 · depth; every launch but the last is full
  for (int depth : {1, 22, 32}) {
    for (int64_t total : {(int64_t)1, (int64_t)depth, (int64_t)depth + 1, (int64_t)3 * depth}) {
      int64_t left = total, launches = 0;
      while (left > 0) {
        const int k = qs::branch_chunk(left, depth);
        CHECK(k >= 1 && k <= depth && k <= left);
        CHECK(k == depth || k == left);
        left -= k;
        launches += 1;
      }
      CHECK(launches == qs::branch_launches(total, depth));
    }
    CHECK(qs::branch_launches(1, depth) == 1 && qs::branch_launches(depth, depth) == 1);
    CHECK(qs::branch_launches((int64_t)depth + 1, depth) == 2 && qs::branch_launches((int64_t)3 * depth, depth) == 3);
  }
  CHECK(qs::branch_chunk(0, 32) == 0 && qs::branch_chunk(-5, 32) == 0 && qs::branch_chunk(5, 0) == 0);
  CHECK(qs::branch_launches(0, 32) == 0 && qs::branch_launches(5, 0) == 0);
  CHECK(qs::branch_chunk(INT64_MAX, 32) == 32);
  CHECK(qs::branch_steps_fit(0, 32) && qs::branch_steps_fit((int64_t)INT32_MAX - 32, 32));
  CHECK(!qs::branch_steps_fit((int64_t)INT32_MAX - 31, 32) && !qs::branch_steps_fit(-1, 1));

  // ---- the live / first-done rule: chains against the straight loop
  const int depth = 32, total = depth + 9;
  std::vector<double> rew(total);
  for (int j = 0; j < total; ++j) rew[j] = 0.1 * (j + 1) - 1.0 / (j + 3);   // sums that round
  const int first_dones[] = {-1, 0, 3, 6, 7, depth - 1, depth, depth + 1, total - 1};
  const std::vector<std::vector<int>> cuts = {{total}, {depth, 9}, {7, 7, total - 14}, {1, 1, total - 2}};
  for (int fd : first_dones) {
    for (int again : {0, 1}) {   // done a second time later: only the first counts
      std::vector<uint8_t> done(total, 0);
      if (fd >= 0) done[fd] = 1;
      if (again && fd >= 0 && fd + 2 < total) done[fd + 2] = 1;
      const qs::BranchAcc want = straight(rew, done);
      CHECK(want.first_done == (fd < 0 ? total : fd));
      for (const auto& cut : cuts) {
        qs::BranchAcc a;   // after a fork: ret 0, first_done 0 = steps
        int64_t t = 0;
        for (int n : cut) {
          qs::branch_accumulate(a, t, n, rew.data() + t, done.data() + t);
          t += n;
        }
        CHECK(t == total);
        CHECK(a.first_done == want.first_done);
        CHECK(std::memcmp(&a.ret, &want.ret, sizeof(double)) == 0);
      }
    }
  }
  std::printf("step_branch ok\n");
  return 0;
}
