// knn_search.h — what the two exact nearest-neighbour searches share (knn.hip: a set against itself; knn_query.hip: one
// set against another): the ONE distance function, the per-lane list of the K best and the wave-uniform scan of a run of
// 16-byte rows [x, y, z, bits of the original index].  Device code only; the kernels stay in their files.
//
// Arithmetic.  d2 = (dx dx + dy dy) + dz dz on float32 coordinate differences, unfused (contraction is off from here to
// the end of the including file): a distance is a pure function of its pair, so the K smallest are bitwise independent
// of scan order, block size and the orders the rows were gathered in.  The AABB distance is the same function on
// clamped differences: float subtraction, max, multiplication and addition are monotone, so it is <= the distance to
// any point inside the box, and a box-to-box distance is <= the AABB distance of any query inside the second box: `<=`
// pruning never drops a neighbour, ties included.
#pragma once

#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace ms {

constexpr int KNN_BLOCK = MS_KNN_BLOCK;
static_assert(KNN_BLOCK == 256, "the gather kernels reduce four waves");

__device__ __forceinline__ float knn_dist2(float dx, float dy, float dz) { return dx * dx + dy * dy + dz * dz; }

// component of the distance from the interval [lo, hi] to the interval [a, b] (a == b: a point); 0 when they overlap
__device__ __forceinline__ float knn_gap(float lo, float hi, float a, float b) { return fmaxf(fmaxf(lo - b, a - hi), 0.0f); }

// the operators of the box reductions (wave_all)
struct KnnMin { __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); } };
struct KnnMax { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };

// The K best of one lane, ascending.  insert() is an unrolled shift with compile-time indices only.
template <int K>
struct KnnBest {
  float d[K];
  int id[K];

  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int s = 0; s < K; ++s) {
      d[s] = INFINITY;
      id[s] = -1;
    }
  }

  __device__ __forceinline__ void insert(float d2, int index) {
#pragma unroll
    for (int s = K - 1; s > 0; --s) {
      const bool above = d2 < d[s - 1], here = d2 < d[s];
      d[s] = above ? d[s - 1] : (here ? d2 : d[s]);
      id[s] = above ? id[s - 1] : (here ? index : id[s]);
    }
    const bool first = d2 < d[0];
    d[0] = first ? d2 : d[0];
    id[0] = first ? index : id[0];
  }
};

// SELF: the row whose index is `self` is skipped (the search of a set against itself); otherwise `self` is not read
template <int K, bool SELF = true>
__device__ __forceinline__ void knn_test(KnnBest<K>& best, float4 c, float4 q, int self) {
  const float d2 = knn_dist2(q.x - c.x, q.y - c.y, q.z - c.z);
  const int index = __float_as_int(c.w);
  if (d2 < best.d[K - 1] && (!SELF || index != self)) best.insert(d2, index);
}

// Every lane tests the `count` rows at the wave-uniform address `rows` against its own list.  The rows are fetched
// KNN_GROUP at a time BEFORE the first test: left to itself the compiler issues one scalar load per row behind the
// previous row's insertion branch and waits for each.
constexpr int KNN_GROUP = 8;

template <int K, bool SELF = true>
__device__ __forceinline__ void knn_scan(KnnBest<K>& best, const float4* __restrict__ rows, int count, float4 q, int self) {
  int j = 0;
  for (; j + KNN_GROUP <= count; j += KNN_GROUP) {
    float4 c[KNN_GROUP];
#pragma unroll
    for (int u = 0; u < KNN_GROUP; ++u) c[u] = rows[j + u];
#pragma unroll
    for (int u = 0; u < KNN_GROUP; ++u) knn_test<K, SELF>(best, c[u], q, self);
  }
  for (; j < count; ++j) knn_test<K, SELF>(best, rows[j], q, self);
}

}  // namespace ms
