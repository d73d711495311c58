// csrc/unionfind.hpp compiled for the host over std::atomic<int32_t>: eight threads unite shuffled edge lists, a flatten follows,
// and the labels must equal a sequential union-find's (the smallest id of every group).  parent[x] <= x is checked after every phase.
//   g++ -O2 -std=c++17 -pthread -o unionfind_check unionfind_check.cpp && ./unionfind_check   -> "failures=0"
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <numeric>
#include <random>
#include <thread>
#include <utility>
#include <vector>

#include "../../semanticlens_amd/csrc/unionfind.hpp"

namespace {

struct HostOps {
  using word = std::atomic<int32_t>;
  static int32_t load(const word* p) { return p->load(std::memory_order_relaxed); }
  static int32_t fetch_min(word* p, int32_t v) {
    int32_t old = p->load(std::memory_order_relaxed);
    while (old > v && !p->compare_exchange_weak(old, v, std::memory_order_relaxed)) {
    }
    return old;
  }
};

using Edges = std::vector<std::pair<int32_t, int32_t>>;
constexpr int kThreadCount = 8;
int failures = 0;

void expect(bool ok, const char* name, const char* what) {
  if (!ok) {
    ++failures;
    std::printf("FAIL %s: %s\n", name, what);
  }
}

bool below_or_self(const std::atomic<int32_t>* parent, int32_t n) {
  for (int32_t x = 0; x < n; ++x) {
    const int32_t p = parent[x].load();
    if (p < 0 || p > x) return false;
  }
  return true;
}

// sequential reference: labels[x] = the smallest id of x's group
std::vector<int32_t> reference(int32_t n, const Edges& edges) {
  std::vector<int32_t> p(n);
  std::iota(p.begin(), p.end(), 0);
  auto root = [&](int32_t x) {
    while (p[x] != x) x = p[x] = p[p[x]];
    return x;
  };
  for (auto [a, b] : edges) {
    const int32_t ra = root(a), rb = root(b);
    if (ra != rb) p[std::max(ra, rb)] = std::min(ra, rb);
  }
  for (int32_t x = 0; x < n; ++x) p[x] = root(x);
  return p;
}

void run(const char* name, int32_t n, const Edges& edges) {
  const std::vector<int32_t> want = reference(n, edges);
  std::unique_ptr<std::atomic<int32_t>[]> parent(new std::atomic<int32_t>[n]);
  for (int32_t x = 0; x < n; ++x) parent[x].store(x);
  std::atomic<int> capped{0};
  {
    std::vector<std::thread> pool;
    for (int t = 0; t < kThreadCount; ++t)
      pool.emplace_back([&, t] {
        for (size_t e = t; e < edges.size(); e += kThreadCount)
          if (!sl::unionfind::unite<HostOps>(parent.get(), edges[e].first, edges[e].second, n)) ++capped;
      });
    for (auto& th : pool) th.join();
  }
  expect(capped.load() == 0, name, "a unite passed its cap");
  expect(below_or_self(parent.get(), n), name, "parent[x] <= x broken after the unites");
  {
    std::vector<std::thread> pool;
    for (int t = 0; t < kThreadCount; ++t)
      pool.emplace_back([&, t] {
        for (int32_t x = t; x < n; x += kThreadCount)
          if (!sl::unionfind::flatten<HostOps>(parent.get(), x, n)) ++capped;
      });
    for (auto& th : pool) th.join();
  }
  expect(capped.load() == 0, name, "a flatten passed its cap");
  expect(below_or_self(parent.get(), n), name, "parent[x] <= x broken after the flatten");
  bool same = true;
  for (int32_t x = 0; x < n; ++x) same = same && parent[x].load() == want[x];
  expect(same, name, "labels differ from the sequential union-find");
  for (int32_t x = 0; x < n; ++x)  // idempotent
    sl::unionfind::flatten<HostOps>(parent.get(), x, n);
  for (int32_t x = 0; x < n; ++x) same = same && parent[x].load() == want[x];
  expect(same, name, "a second flatten changed the labels");
}

Edges shuffled(Edges e, uint32_t seed) {
  std::mt19937 rng(seed);
  std::shuffle(e.begin(), e.end(), rng);
  for (auto& p : e)
    if (rng() & 1) std::swap(p.first, p.second);
  return e;
}

}  // namespace

int main() {
  std::mt19937 rng(7);
  {  // a random sparse graph on 10 000 ids: about 0.6 edges per id, many small groups and some large ones
    const int32_t n = 10000;
    std::uniform_int_distribution<int32_t> id(0, n - 1);
    Edges e;
    for (int i = 0; i < 6000; ++i) e.emplace_back(id(rng), id(rng));  // self loops included
    run("sparse", n, shuffled(e, 1));
  }
  {  // a 1 000-clique among 1 500 ids: every unite contends for the same few roots
    Edges e;
    for (int32_t a = 200; a < 1200; ++a)
      for (int32_t b = a + 1; b < 1200; ++b) e.emplace_back(a, b);
    run("clique", 1500, shuffled(e, 2));
  }
  {  // a 5 000-chain given in reverse order: the deepest trees the hook rule can build
    Edges e;
    for (int32_t a = 4999; a > 0; --a) e.emplace_back(a, a - 1);
    run("chain", 5000, e);
    run("chain shuffled", 5000, shuffled(e, 3));
  }
  run("empty", 100, Edges{});
  std::printf("failures=%d\n", failures);
  return failures != 0;
}
