// Host-side check of semanticlens_amd/csrc/reduce_policy.hpp: nt_head_units / nt_policy_applies on a resolved policy.
// Built and run by tests/test_host_logic.py with g++.
#include <cstdint>
#include <cstdio>

#include "../../semanticlens_amd/csrc/reduce_policy.hpp"

static int failures = 0;
#define CHECK_EQ(got, want)                                                                                \
  do {                                                                                                     \
    const long long g_ = (long long)(got), w_ = (long long)(want);                                         \
    if (g_ != w_) {                                                                                        \
      std::printf("line %d: %s = %lld, expected %lld\n", __LINE__, #got, g_, w_);                          \
      ++failures;                                                                                          \
    }                                                                                                      \
  } while (0)

int main() {
  using sl::ReducePolicy;
  constexpr int64_t MiB = (int64_t)1 << 20;
  // the built-in default: 300 MiB keep a 240 MiB tail, 255 MiB are below the threshold
  const ReducePolicy dflt{256 * MiB, 240 * MiB};
  CHECK_EQ(sl::nt_head_units(dflt, 300 * MiB, MiB, 1), 60);
  CHECK_EQ(sl::nt_head_units(dflt, 255 * MiB, MiB, 1), 0);
  CHECK_EQ(sl::nt_policy_applies(dflt, 255 * MiB), false);
  // (0, 0): everything nt
  CHECK_EQ(sl::nt_head_units(ReducePolicy{0, 0}, 1, 1), INT64_MAX);
  // whole units only, then `scale` walk units per unit: (32 - 8) / 3 = 8 units of 4
  const ReducePolicy small{16 * MiB, 8 * MiB};
  CHECK_EQ(sl::nt_head_units(small, 32 * MiB, 3 * MiB, 4), 32);
  // tail_cap below tail_bytes: the tail is the cap
  CHECK_EQ(sl::nt_head_units(small, 32 * MiB, MiB, 1, 2 * MiB), 30);
  // the nt instance with the whole input as tail
  const ReducePolicy all_tail{1 * MiB, 64 * MiB};
  CHECK_EQ(sl::nt_head_units(all_tail, 32 * MiB, MiB, 1), 0);
  CHECK_EQ(sl::nt_policy_applies(all_tail, 32 * MiB), true);
  std::printf("failures=%d\n", failures);
  return failures ? 1 : 0;
}
