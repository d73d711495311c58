// K1 / K2 — cache policy of the reduce streams: a value that travels with every call (ReduceCall, reduce_common.hpp).
// Needs only <cstdint>: a host compiler can include it (tests/native/reduce_policy_check.cpp).
//
// A COLD input streams best with the nt (read-once) policy: 6.4 vs 5.9 TB/s on 411 MB.  Inside a model the input was
// written by the previous kernel microseconds ago; what still sits (dirty) in the 256 MiB Infinity Cache reads faster
// with the default policy and nt on it LOSES (in-bench average 5.0 TB/s all-nt vs 5.9 mixed).  The kernel cannot know
// its producer, so the default assumes the common case — a forward hook on the layer that just ran: inputs below
// `nt_min_bytes` (default 256 MiB) are read with the default policy; of larger ones the last `tail_bytes` (default
// 240 MiB: what the cache still holds) likewise and the head with nt.  tail_bytes = 0 and nt_min_bytes = 0 = all nt,
// the right setting for inputs known to be cold.  The kernels walk the tail FIRST — the most recently written bytes are
// read while the cache still holds them (in-pipeline 411 MB: 6.07 -> 6.44 TB/s) — and inputs read entirely with the default
// policy front to back.
#pragma once
#include <cstdint>

namespace sl {

// Resolved: both fields >= 0.  At the C boundary a negative field means the process default (sl_set_reduce_policy, or the
// environment SL_NT_MIN_BYTES / SL_REDUCE_TAIL_MB); reduce.hip resolves it once per call, before any dispatch.
struct ReducePolicy {
  int64_t nt_min_bytes, tail_bytes;
};

// true: the input is large enough (>= nt_min_bytes) for the nt / default split
inline bool nt_policy_applies(const ReducePolicy& p, int64_t bytes) { return bytes >= p.nt_min_bytes; }

// How many leading walk units of an input of `bytes` bytes are read with nt; the rest — the last min(tail_bytes, tail_cap)
// bytes, what the Infinity Cache may still hold — with the default policy.  `unit_bytes` is the byte size of the kernel's
// unit, `scale` the walk units per such unit.  0 = all default (input below nt_min_bytes or not longer than the tail),
// INT64_MAX = all nt (tail_bytes = 0).
inline int64_t nt_head_units(const ReducePolicy& p, int64_t bytes, int64_t unit_bytes, int64_t scale = 1,
                             int64_t tail_cap = INT64_MAX) {
  if (!nt_policy_applies(p, bytes)) return 0;
  const int64_t tail = p.tail_bytes < tail_cap ? p.tail_bytes : tail_cap;
  if (tail <= 0) return INT64_MAX;
  return bytes > tail ? (bytes - tail) / unit_bytes * scale : 0;
}

}  // namespace sl
