// Host-side check of semanticlens_amd/csrc/kmeans_layout.hpp: the one description of where K9 keeps a component's state, used by
// the kernels' carve-up and by the size queries.  Built and run by tests/test_host_logic.py with g++.
// The size table was recorded from sl_poly2means_ws_bytes / sl_polykmeans_ws_bytes before the header took the formulas over:
// Python chunks components by these values, so they must not move.
#include <cstdint>
#include <cstdio>

#include "../../semanticlens_amd/csrc/kmeans_layout.hpp"

using namespace sl::k9;

static int failures = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      if (++failures <= 20) {                  \
        std::printf("line %d: ", __LINE__);    \
        std::printf(__VA_ARGS__);              \
        std::printf("\n");                     \
      }                                        \
    }                                          \
  } while (0)

struct Recorded {
  int64_t C, n;
  int k, n_init;
  unsigned long long polyk, poly2;  // poly2 == 0: outside the LDS variant (k != 2 or n > 128)
};

// every array starts where the one before it ends, in the documented order, and `end` is the last one's end
static void check_carve(const Layout& L, int64_t n, int64_t k, bool keeps_r, int64_t cand_rows) {
  const size_t N = (size_t)n, K = (size_t)k;
  const size_t starts[] = {L.G, L.r, L.s, L.sn, L.closest, L.cand, L.label, L.label_old, L.member, L.best_label, L.best_member, L.end};
  const size_t sizes[] = {N * N * 8, keeps_r ? N * 8 : 0, K * N * 8, K * N * 8, N * 8, (size_t)cand_rows * N * 8, N * 4, N * 4, N * 4, N * 4, N * 4};
  CHECK(L.G == 0, "n %lld k %lld: G starts at %zu", (long long)n, (long long)k, L.G);
  for (int a = 0; a < 11; ++a)
    CHECK(starts[a] + sizes[a] == starts[a + 1], "n %lld k %lld: array %d [%zu, +%zu) is not followed by the next at %zu", (long long)n,
          (long long)k, a, starts[a], sizes[a], starts[a + 1]);
  for (int a = 0; a < 6; ++a) CHECK(starts[a] % 8 == 0, "n %lld k %lld: double array %d is not 8-byte aligned", (long long)n, (long long)k, a);
}

int main() {
  static const Recorded table[] = {
      {1, 2, 2, 10, 1312ull, 288ull},            {7, 2, 2, 32, 3808ull, 480ull},           {1, 20, 2, 10, 9344ull, 3456ull},
      {7, 20, 2, 32, 60032ull, 22656ull},        {1, 20, 3, 10, 9856ull, 0ull},            {7, 20, 3, 32, 62848ull, 0ull},
      {1, 20, 16, 10, 18304ull, 0ull},           {7, 20, 16, 32, 106624ull, 0ull},         {1, 128, 2, 10, 274944ull, 131328ull},
      {7, 128, 2, 32, 1919232ull, 917760ull},    {1, 128, 3, 10, 277248ull, 0ull},         {7, 128, 3, 32, 1934592ull, 0ull},
      {1, 128, 16, 10, 307968ull, 0ull},         {7, 128, 16, 32, 2134272ull, 0ull},       {1, 1024, 2, 10, 16872448ull, 0ull},
      {7, 1024, 2, 32, 118101760ull, 0ull},      {1, 1024, 3, 10, 16889088ull, 0ull},      {7, 1024, 3, 32, 118217472ull, 0ull},
      {1, 1024, 16, 10, 17106176ull, 0ull},      {7, 1024, 16, 32, 119721728ull, 0ull}};
  for (const Recorded& t : table) {
    CHECK(polykmeans_ws_bytes(t.C, t.n, t.k, t.n_init) == t.polyk, "polykmeans_ws_bytes(%lld, %lld, %d, %d) = %zu, recorded %llu",
          (long long)t.C, (long long)t.n, t.k, t.n_init, polykmeans_ws_bytes(t.C, t.n, t.k, t.n_init), t.polyk);
    if (t.poly2)
      CHECK(poly2means_ws_bytes(t.C, t.n) == t.poly2, "poly2means_ws_bytes(%lld, %lld) = %zu, recorded %llu", (long long)t.C,
            (long long)t.n, poly2means_ws_bytes(t.C, t.n), t.poly2);
    // the workspace variant's carve-up ends inside the slice the size query reports, less than one 256-byte step before its end
    const Layout W = ws_layout(t.n, t.k);
    check_carve(W, t.n, t.k, false, kMaxTrials);
    CHECK(W.end <= ws_slice_bytes(t.n, t.k) && ws_slice_bytes(t.n, t.k) - W.end < 256 && ws_slice_bytes(t.n, t.k) % 256 == 0,
          "n %lld k %d: the slice is %zu bytes, the carve-up ends at %zu", (long long)t.n, t.k, ws_slice_bytes(t.n, t.k), W.end);
    if (t.n <= kLdsMaxN) {  // the LDS variant's carve-up ends exactly at the dynamic LDS size the launch asks for
      const Layout L = lds_layout(t.n);
      check_carve(L, t.n, 2, true, 0);
      CHECK(L.end == lds_bytes(t.n), "n %lld: lds_bytes %zu, the carve-up ends at %zu", (long long)t.n, lds_bytes(t.n), L.end);
    }
  }
  // the LDS variant at its limit fits a CU's 160 KiB with the kernel's static LDS (the per-cluster scalars: well under 1 KiB)
  static_assert(kLdsMaxN == 128 && lds_bytes(kLdsMaxN) + 1024 <= 160 * 1024, "the LDS variant at n = 128 must fit 160 KiB");
  static_assert(lds_bytes(20) == 4560 && lds_bytes(128) == 139776, "dynamic LDS per component at n = 20 / n = 128");
  static_assert(kMaxClusters == 16 && kMaxNGeneral == 1024 && kMaxTrials == 4, "the limits _native.py and the messages state");

  std::printf("failures=%d\n", failures);
  return failures ? 1 : 0;
}
