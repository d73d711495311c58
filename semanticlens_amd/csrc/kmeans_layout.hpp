// K9 — where one component's k-means state lives, and how much room a call needs (csrc/kmeans.hip).
//
// The procedure is written once; its state is a list of arrays carved out of one block of bytes.  The block is dynamic LDS
// in the LDS variant (k = 2, n <= kLdsMaxN) and a slice of the caller's workspace in the workspace variant (k <= kMaxClusters,
// n <= kMaxNGeneral).  `layout()` is the one description of that list: the kernel carves with it, the host sizes with it.
// Plain constexpr C++: tests/native/kmeans_layout_check.cpp compiles it with g++ and pins the sizes.
#pragma once
#include <cstddef>
#include <cstdint>

namespace sl {
namespace k9 {

constexpr int kLdsMaxN = 128;       // LDS variant: samples per component
constexpr int kMaxClusters = 16;    // workspace variant: n_clusters
constexpr int kMaxNGeneral = 1024;  // workspace variant: samples per component
constexpr int kMaxTrials = 4;       // 2 + int(ln kMaxClusters) k-means++ candidates per further centre

// Byte offsets of one component's arrays.  doubles first, then the int arrays; every array is n-major.
struct Layout {
  size_t G;         // n x n   centred Gram matrix
  size_t r;         // n       r_i = mean_j H_ij (the fallback score reads it); absent (== s) where it is re-summed from H
  size_t s;         // k x n   sum_{l in S_j} G_il of the current member sets
  size_t sn;        // k x n   the same for the next member sets; its first n doubles double as the relocation's distances
  size_t closest;   // n       k-means++: squared distance to the nearest centre so far (r_i is parked here while G is built)
  size_t cand;      // t x n   k-means++: the same under each candidate, kept only while further centres follow
  size_t label, label_old, member, best_label, best_member;  // n ints each
  size_t end;       // bytes used
};

constexpr Layout layout(int64_t n, int64_t k, bool keeps_r, int64_t cand_rows) {
  Layout L{};
  size_t at = 0;
  const size_t N = (size_t)n, K = (size_t)k;
  L.G = at; at += N * N * 8;
  L.r = at; at += keeps_r ? N * 8 : 0;
  L.s = at; at += K * N * 8;
  L.sn = at; at += K * N * 8;
  L.closest = at; at += N * 8;
  L.cand = at; at += (size_t)cand_rows * N * 8;
  L.label = at; at += N * 4;
  L.label_old = at; at += N * 4;
  L.member = at; at += N * 4;
  L.best_label = at; at += N * 4;
  L.best_member = at; at += N * 4;
  L.end = at;
  return L;
}

// LDS variant: k = 2 is the last centre k-means++ seeds, so no candidate rows; r_i stays resident.
constexpr Layout lds_layout(int64_t n) { return layout(n, 2, true, 0); }
constexpr size_t lds_bytes(int64_t n) { return lds_layout(n).end; }

// Workspace variant: one slice per component, a multiple of 256 bytes.
constexpr Layout ws_layout(int64_t n, int64_t k) { return layout(n, k, false, kMaxTrials); }
constexpr size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
constexpr size_t ws_slice_bytes(int64_t n, int64_t k) { return align256(ws_layout(n, k).end); }

// What the callers allocate (sl_poly2means_ws_bytes / sl_polykmeans_ws_bytes): the fp64 Gram matrices, then for the workspace
// variant the slices and the device copy of the draws.  Python chunks the component axis by these.
constexpr size_t poly2means_ws_bytes(int64_t C, int64_t n) { return (size_t)C * (size_t)n * (size_t)n * 8 + 256; }
constexpr size_t draws_bytes(int n_init, int k) {
  return (size_t)n_init * 4 + (size_t)n_init * (size_t)(k > 1 ? k - 1 : 1) * kMaxTrials * 8;
}
constexpr size_t polykmeans_ws_bytes(int64_t C, int64_t n, int k, int n_init) {
  return (size_t)C * (size_t)n * (size_t)n * 8 + (size_t)C * ws_slice_bytes(n, k) + align256(draws_bytes(n_init, k)) + 512;
}

}  // namespace k9
}  // namespace sl
