// knn_query.hip — exact k nearest POINTS of every QUERY, two different 3D sets (1 <= k <= 8): the search behind
// surface_distances / surface_metrics (Chamfer distance, precision / recall / F-score of a mesh against a ground-truth
// cloud), colour transfer between clouds and "drop what lies farther than d from the surface".  The design of knn.hip
// with a second set: the points are gathered into blocks with boxes, the queries ride one per lane in their own order.
// Nothing is excluded: a query that coincides with a point finds it at distance 0.
//
//   knn_query_gather_kernel    points through `point_order` into 16-byte rows [x, y, z, bits of the original index];
//                              every run of KNN_BLOCK rows is a block, and the workgroup that gathers it reduces its
//                              AABB (__shfl_xor inside a wave, 96 bytes of LDS across the four waves).
//   knn_query_search_kernel<K> one lane per query, in `query_order`, so the 64 queries of a wave are neighbours in
//                              space; the query itself is read through the order (one 12-byte gather per lane).  The
//                              wave seeds its lists from ONE block: the one that holds position
//                              clamp(query_hint[i], 0, m - 1) of point_order for i = the wave's middle active lane
//                              (i m / n without a hint) — a wave-uniform load.  Then it walks every chunk of 64 block
//                              boxes outward from the seed, as knn_search_kernel does: each lane tests one block's AABB
//                              against the wave's own box and largest K-th best, the ballot of that is the candidate
//                              list; a candidate is scanned when ANY lane's distance to the AABB is <= that lane's
//                              K-th best.  Every decision is wave-uniform, so the rows of a scanned block are read at
//                              wave-uniform addresses (scalar loads).  Every chunk is visited and every pruning test
//                              is `<=`: the hint and the two orders decide the speed, never the result.  No LDS, no
//                              barrier, no atomics but the optional counters; m == 0 writes +inf / -1.
//
// Arithmetic: knn_search.h — the distance function of knn.hip, unfused.
#include "knn_search.h"

namespace ms {

struct KnnQueryScratch {
  size_t rows, lo, hi, total;
};

static KnnQueryScratch knn_query_scratch(int64_t m) {
  const size_t blocks = (size_t)div_up(m, KNN_BLOCK);
  Carve c;
  KnnQueryScratch s;
  s.rows = c.take((size_t)m * sizeof(float4));
  s.lo = c.take(blocks * sizeof(float4));
  s.hi = c.take(blocks * sizeof(float4));
  s.total = c.off;
  return s;
}

__global__ void __launch_bounds__(KNN_BLOCK)
knn_query_gather_kernel(const float* __restrict__ points, const int32_t* __restrict__ order, int m,
                        float4* __restrict__ rows, float4* __restrict__ block_lo, float4* __restrict__ block_hi) {
  __shared__ float part[KNN_BLOCK / WAVE][6];
  const int64_t i = (int64_t)blockIdx.x * KNN_BLOCK + (int64_t)threadIdx.x;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < m) {
    // `order` is a permutation by contract; an index outside 0..m-1 is clamped so that no access leaves the arrays
    const int src = min(max(order[i], 0), m - 1);
    const float x = points[(int64_t)src * 3 + 0], y = points[(int64_t)src * 3 + 1], z = points[(int64_t)src * 3 + 2];
    rows[i] = make_float4(x, y, z, __int_as_float(src));
    lo[0] = hi[0] = x;
    lo[1] = hi[1] = y;
    lo[2] = hi[2] = z;
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = wave_all(lo[a], KnnMin());
    hi[a] = wave_all(hi[a], KnnMax());
    if (lane_id() == 0) {
      part[wave][a] = lo[a];
      part[wave][3 + a] = hi[a];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float r[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) r[a] = part[0][a];
#pragma unroll
    for (int w = 1; w < KNN_BLOCK / WAVE; ++w) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        r[a] = fminf(r[a], part[w][a]);
        r[3 + a] = fmaxf(r[3 + a], part[w][3 + a]);
      }
    }
    block_lo[blockIdx.x] = make_float4(r[0], r[1], r[2], 0.0f);
    block_hi[blockIdx.x] = make_float4(r[3], r[4], r[5], 0.0f);
  }
}

template <int K>
__global__ void __launch_bounds__(KNN_BLOCK)
knn_query_search_kernel(const float4* __restrict__ rows, const float4* __restrict__ block_lo,
                        const float4* __restrict__ block_hi, int m, int blocks, const float* __restrict__ queries,
                        const int32_t* __restrict__ query_order, const int32_t* __restrict__ query_hint, int n,
                        float* __restrict__ out_dist2, int32_t* __restrict__ out_index,
                        unsigned long long* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * KNN_BLOCK + (int64_t)threadIdx.x;
  const bool active = i < n;
  const unsigned long long active_mask = __ballot(active);
  if (active_mask == 0) return;                     // a whole wave past the end (the waves never meet at a barrier)
  const int lanes = __popcll(active_mask);          // the active lanes are 0 .. lanes - 1
  // idle lanes follow along with the last query and store nothing; an entry of the order outside 0..n-1 is clamped
  const int self = min(max(query_order[active ? i : (int64_t)n - 1], 0), n - 1);
  const float4 q = make_float4(queries[(int64_t)self * 3 + 0], queries[(int64_t)self * 3 + 1],
                               queries[(int64_t)self * 3 + 2], 0.0f);

  KnnBest<K> best;
  best.clear();
  unsigned long long scanned = 0, evaluated = 0;

  if (blocks > 0) {
    // the seed: the block of the hinted position of the wave's middle active lane, the same in every lane
    const int64_t middle = i - (int64_t)lane_id() + (int64_t)(lanes >> 1);
    const int64_t hinted = query_hint != nullptr ? (int64_t)query_hint[middle] : middle * (int64_t)m / (int64_t)n;
    const int64_t position = min(max(hinted, (int64_t)0), (int64_t)m - 1);
    const int seed = __builtin_amdgcn_readfirstlane((int)(position / KNN_BLOCK));
    const int seed_count = min(KNN_BLOCK, m - seed * KNN_BLOCK);
    knn_scan<K, false>(best, rows + (int64_t)seed * KNN_BLOCK, seed_count, q, 0);
    scanned = (unsigned long long)lanes;
    evaluated = (unsigned long long)lanes * (unsigned long long)seed_count;

    // the box of this wave's queries
    float wlo[3], whi[3];
    wlo[0] = wave_all(active ? q.x : INFINITY, KnnMin());
    wlo[1] = wave_all(active ? q.y : INFINITY, KnnMin());
    wlo[2] = wave_all(active ? q.z : INFINITY, KnnMin());
    whi[0] = wave_all(active ? q.x : -INFINITY, KnnMax());
    whi[1] = wave_all(active ? q.y : -INFINITY, KnnMax());
    whi[2] = wave_all(active ? q.z : -INFINITY, KnnMax());

    // the other blocks, 64 per step, outward from the seed along the curve: its chunk, +1, -1, +2, -2, ...
    const int chunks = (blocks + WAVE - 1) / WAVE, seed_chunk = seed / WAVE;
    const int steps = 2 * max(seed_chunk, chunks - 1 - seed_chunk);
    for (int t = 0; t <= steps; ++t) {
      const int off = (t + 1) >> 1;
      const int chunk = (t & 1) ? seed_chunk + off : seed_chunk - off;
      if (chunk < 0 || chunk >= chunks) continue;
      // candidates: the block's box against the wave's box and the wave's largest K-th best (each lane one block)
      const float reach = wave_all(active ? best.d[K - 1] : -INFINITY, KnnMax());
      const int b = chunk * WAVE + lane_id();
      bool candidate = false;
      if (b < blocks && b != seed) {
        const float4 lo = block_lo[b], hi = block_hi[b];
        candidate = knn_dist2(knn_gap(lo.x, hi.x, wlo[0], whi[0]), knn_gap(lo.y, hi.y, wlo[1], whi[1]),
                              knn_gap(lo.z, hi.z, wlo[2], whi[2])) <= reach;
      }
      unsigned long long todo = __ballot(candidate);
      while (todo != 0) {
        const int blk = __builtin_amdgcn_readfirstlane(chunk * WAVE + (__ffsll((long long)todo) - 1));
        todo &= todo - 1;
        const float4 lo = block_lo[blk], hi = block_hi[blk];
        const float box2 = knn_dist2(knn_gap(lo.x, hi.x, q.x, q.x), knn_gap(lo.y, hi.y, q.y, q.y), knn_gap(lo.z, hi.z, q.z, q.z));
        if (__ballot(active && box2 <= best.d[K - 1]) == 0) continue;
        const int count = min(KNN_BLOCK, m - blk * KNN_BLOCK);
        knn_scan<K, false>(best, rows + (int64_t)blk * KNN_BLOCK, count, q, 0);
        scanned += (unsigned long long)lanes;
        evaluated += (unsigned long long)lanes * (unsigned long long)count;
      }
    }
  }

  if (active) {
#pragma unroll
    for (int s = 0; s < K; ++s) out_dist2[(int64_t)self * K + s] = best.d[s];
    if (out_index != nullptr) {
#pragma unroll
      for (int s = 0; s < K; ++s) out_index[(int64_t)self * K + s] = best.id[s];
    }
  }
  if (stats != nullptr && lane_id() == 0 && blocks > 0) {     // lane 0 of a wave that got here is active
    atomicAdd(stats + 0, scanned);
    atomicAdd(stats + 1, evaluated);
  }
}

template <int K>
static void knn_query_launch(const float4* rows, const float4* lo, const float4* hi, int m, int blocks, const float* queries,
                             const int32_t* query_order, const int32_t* query_hint, int n, float* out_dist2,
                             int32_t* out_index, int64_t* out_stats, hipStream_t stream) {
  knn_query_search_kernel<K><<<(unsigned)div_up(n, KNN_BLOCK), KNN_BLOCK, 0, stream>>>(
    rows, lo, hi, m, blocks, queries, query_order, query_hint, n, out_dist2, out_index, (unsigned long long*)out_stats);
}

}  // namespace ms

using namespace ms;

extern "C" int ms_knn_query(const float* points3, const int32_t* point_order, int64_t m, const float* queries3,
                            const int32_t* query_order, const int32_t* query_hint, int64_t n, int k, float* out_dist2,
                            int32_t* out_index, int64_t* out_stats, void* tmp, size_t* tmp_bytes, void* stream) {
  MS_CHECK_ARG(m >= 0 && n >= 0, "m < 0 or n < 0");
  MS_CHECK_ARG(m < ((int64_t)1 << 31) && n < ((int64_t)1 << 31), "m >= 2^31 or n >= 2^31 (indices are int32)");
  MS_CHECK_ARG(k >= 1 && k <= 8, "k must be in 1..8");
  const KnnQueryScratch s = knn_query_scratch(m);
  MS_CHECK_TMP(tmp, tmp_bytes, s.total);
  if (n == 0) return 0;
  MS_CHECK_ARG(m == 0 || (points3 != nullptr && point_order != nullptr), "points3 or point_order is null");
  MS_CHECK_ARG(queries3 != nullptr && query_order != nullptr, "queries3 or query_order is null");
  MS_CHECK_ARG(out_dist2 != nullptr, "out_dist2 is null");
  MS_CHECK_ARG(aligned(16, {tmp}), "tmp must be aligned to 16 bytes (float4 rows)");

  float4* rows = at<float4>(tmp, s.rows);
  float4* lo = at<float4>(tmp, s.lo);
  float4* hi = at<float4>(tmp, s.hi);
  const int blocks = (int)div_up(m, KNN_BLOCK);
  hipStream_t st = (hipStream_t)stream;
  if (m > 0) {
    knn_query_gather_kernel<<<(unsigned)blocks, KNN_BLOCK, 0, st>>>(points3, point_order, (int)m, rows, lo, hi);
    MS_CHECK_LAUNCH();
  }
  const int mi = (int)m, ni = (int)n;
  switch (k) {
    case 1: knn_query_launch<1>(rows, lo, hi, mi, blocks, queries3, query_order, query_hint, ni, out_dist2, out_index, out_stats, st); break;
    case 2: knn_query_launch<2>(rows, lo, hi, mi, blocks, queries3, query_order, query_hint, ni, out_dist2, out_index, out_stats, st); break;
    case 3: knn_query_launch<3>(rows, lo, hi, mi, blocks, queries3, query_order, query_hint, ni, out_dist2, out_index, out_stats, st); break;
    case 4: knn_query_launch<4>(rows, lo, hi, mi, blocks, queries3, query_order, query_hint, ni, out_dist2, out_index, out_stats, st); break;
    case 5: knn_query_launch<5>(rows, lo, hi, mi, blocks, queries3, query_order, query_hint, ni, out_dist2, out_index, out_stats, st); break;
    case 6: knn_query_launch<6>(rows, lo, hi, mi, blocks, queries3, query_order, query_hint, ni, out_dist2, out_index, out_stats, st); break;
    case 7: knn_query_launch<7>(rows, lo, hi, mi, blocks, queries3, query_order, query_hint, ni, out_dist2, out_index, out_stats, st); break;
    default: knn_query_launch<8>(rows, lo, hi, mi, blocks, queries3, query_order, query_hint, ni, out_dist2, out_index, out_stats, st); break;
  }
  MS_CHECK_LAUNCH();
  return 0;
}
