// The union-find forest of K24 (redgroups.hip) as templates over a small atomic-ops policy.  Needs only <cstdint>: the device
// passes the HIP atomics, a host program passes std::atomic<int32_t> (tests/native/unionfind_check.cpp unites edge lists from
// eight threads with it), so the rule below is checkable on the CPU, as packed_best.hpp's order is.
//
// State: parent[0, n), empty when parent[i] == i.  Invariant: parent[x] <= x at every instant, whatever is running.  It holds
// in the empty state and the only write is fetch_min(&parent[x], v) with v < x, which lowers an entry.  So every walk up the
// parents descends strictly until it meets a root (parent[r] == r): the forest has no cycles, find takes at most n steps
// whatever it races with, and the root of a finished group is its smallest id, which makes the labels deterministic.
//
// Policy: struct Ops { using word = ...; static int32_t load(const word*); static int32_t fetch_min(word*, int32_t); } —
// a relaxed load and a relaxed atomic minimum that returns the entry's previous value.  A stale load can only return a value
// the entry held earlier: an older ancestor, not above x and in x's group.  While unites run, find is therefore only a
// shortcut to a member near the root, and what makes unite right is the value fetch_min returns.  flatten runs with no unite
// in flight (the device: a launch of its own), when the roots are fixed and visible, so its find ends at the true root.
//
// unite(a, b), hi = max, lo = min of the current pair: old = fetch_min(&parent[hi], lo).
//   old == hi: hi was a root and hangs under lo now: done.
//   old != hi: hi had the parent old < hi.  Either the entry kept old (old <= lo) or it now says lo and the link hi - old is
//   gone; in both cases hi is tied to one of the two and what is left to do is unite(old, lo).  Both old and lo are below hi, so
//   the larger id of the pair strictly decreases per iteration: at most n iterations, no waiting on any other thread.
// Every loop still carries the cap n + 1; a caller that sees `false` raises its status word and leaves.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SL_UF_FN __host__ __device__ inline
#else
#define SL_UF_FN inline
#endif

namespace sl {
namespace unionfind {

// the root above x, or the node the cap stopped at (ok = false)
template <class Ops>
SL_UF_FN int32_t find(typename Ops::word* parent, int32_t x, int32_t n, bool& ok) {
  for (int64_t it = 0; it <= (int64_t)n; ++it) {
    const int32_t p = Ops::load(parent + x);
    if (p == x) return x;
    x = p;
  }
  ok = false;
  return x;
}

// join the groups of a and b; false when a loop ran past its cap (cannot happen while the invariant holds)
template <class Ops>
SL_UF_FN bool unite(typename Ops::word* parent, int32_t a, int32_t b, int32_t n) {
  bool ok = true;
  a = find<Ops>(parent, a, n, ok);
  b = find<Ops>(parent, b, n, ok);
  for (int64_t it = 0; ok && it <= (int64_t)n; ++it) {
    if (a == b) return true;
    const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const int32_t old = Ops::fetch_min(parent + hi, lo);
    if (old == hi) return true;
    a = find<Ops>(parent, old, n, ok);  // find(old) <= old < hi
    b = lo;
  }
  return false;
}

// parent[x] = its root; idempotent, and right while other lanes flatten (roots do not move without a unite)
template <class Ops>
SL_UF_FN bool flatten(typename Ops::word* parent, int32_t x, int32_t n) {
  bool ok = true;
  const int32_t r = find<Ops>(parent, x, n, ok);
  if (ok && r != x) Ops::fetch_min(parent + x, r);
  return ok;
}

}  // namespace unionfind
}  // namespace sl
