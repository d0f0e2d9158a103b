// knn.hip — exact k nearest neighbours of every point of a 3D point set among the other points of the same set
// (1 <= k <= 8): the search behind Gaussians3D.from_point_cloud (upstream trainers: simple_knn.distCUDA2; no
// reference counterpart).  The consumer of ms_morton_codes64 + ms_radix_sort_pairs: the points arrive with `order`, a
// permutation (normally their Morton argsort) that only decides how well the search prunes, never what it returns.
//
//   knn_gather_blocks_kernel   points through `order` into 16-byte rows [x, y, z, bits of the original index]; every
//                              run of KNN_BLOCK rows is a block, and the workgroup that gathers it reduces its AABB
//                              (__shfl_xor inside a wave, 96 bytes of LDS across the four waves).
//   knn_search_kernel<K>       one lane per query in sorted order, so the 64 queries of a wave are neighbours in
//                              space.  A lane keeps its K best (d2, index) in registers (an unrolled insertion, K a
//                              template parameter: no indexed array, no scratch).  The wave seeds from its own block,
//                              then walks the other blocks outward along the curve, 64 at a time: each lane tests one
//                              block's AABB against the wave's own box and largest K-th best, the ballot of that is the
//                              candidate list; a candidate is scanned when ANY lane's distance to the AABB is <= that
//                              lane's K-th best.  Every decision is wave-uniform, so the rows of a scanned block are
//                              read at wave-uniform addresses (scalar loads) and each lane tests every row.  No LDS,
//                              no barrier: the waves of a workgroup are independent.
//
// Arithmetic.  d2 = (dx dx + dy dy) + dz dz on float32 coordinate differences, unfused (contraction is off for the
// whole file), in ONE function: a distance is a pure function of its pair, so the K smallest are bitwise independent of
// scan order, block size and `order`.  The AABB distance is the same function on clamped differences: float
// subtraction, max, multiplication and addition are monotone, so it is <= the distance to any point inside the box, and
// the box-to-box distance of the candidate test is <= the AABB distance of any query inside the wave's box: `<=`
// pruning never drops a neighbour, ties included.  Self is excluded by original index, never by distance.
#include "knn_search.h"   // knn_dist2, knn_gap, KnnBest, knn_scan: shared with knn_query.hip

namespace ms {

struct KnnScratch {
  size_t rows, lo, hi, total;
};

static KnnScratch knn_scratch(int64_t n) {
  const size_t blocks = (size_t)div_up(n, KNN_BLOCK);
  Carve c;
  KnnScratch s;
  s.rows = c.take((size_t)n * sizeof(float4));
  s.lo = c.take(blocks * sizeof(float4));
  s.hi = c.take(blocks * sizeof(float4));
  s.total = c.off;
  return s;
}

__global__ void __launch_bounds__(KNN_BLOCK)
knn_gather_blocks_kernel(const float* __restrict__ points, const int32_t* __restrict__ order, int n,
                         float4* __restrict__ rows, float4* __restrict__ block_lo, float4* __restrict__ block_hi) {
  __shared__ float part[KNN_BLOCK / WAVE][6];
  const int i = (int)blockIdx.x * KNN_BLOCK + (int)threadIdx.x;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < n) {
    // `order` is a permutation by contract; an index outside 0..n-1 is clamped so that no access leaves the arrays
    const int src = min(max(order[i], 0), n - 1);
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
knn_search_kernel(const float4* __restrict__ rows, const float4* __restrict__ block_lo, const float4* __restrict__ block_hi,
                  int n, int blocks, float* __restrict__ out_dist2, int32_t* __restrict__ out_index,
                  unsigned long long* __restrict__ stats) {
  const int own = (int)blockIdx.x;
  const int i = own * KNN_BLOCK + (int)threadIdx.x;
  const bool active = i < n;
  const unsigned long long active_mask = __ballot(active);
  if (active_mask == 0) return;                     // a whole wave past the end (the waves never meet at a barrier)
  const int lanes = __popcll(active_mask);
  const float4 q = rows[active ? i : n - 1];       // idle lanes follow along with a valid point and store nothing
  const int self = __float_as_int(q.w);

  KnnBest<K> best;
  best.clear();
  const int own_count = min(KNN_BLOCK, n - own * KNN_BLOCK);
  knn_scan<K>(best, rows + (int64_t)own * KNN_BLOCK, own_count, q, self);
  unsigned long long scanned = (unsigned long long)lanes;
  unsigned long long evaluated = (unsigned long long)lanes * (unsigned long long)(own_count - 1);

  // the box of this wave's queries
  float wlo[3], whi[3];
  wlo[0] = wave_all(active ? q.x : INFINITY, KnnMin());
  wlo[1] = wave_all(active ? q.y : INFINITY, KnnMin());
  wlo[2] = wave_all(active ? q.z : INFINITY, KnnMin());
  whi[0] = wave_all(active ? q.x : -INFINITY, KnnMax());
  whi[1] = wave_all(active ? q.y : -INFINITY, KnnMax());
  whi[2] = wave_all(active ? q.z : -INFINITY, KnnMax());

  // the other blocks, 64 per step, outward from the own one along the curve: own chunk, +1, -1, +2, -2, ...
  const int chunks = (blocks + WAVE - 1) / WAVE, own_chunk = own / WAVE;
  const int steps = 2 * max(own_chunk, chunks - 1 - own_chunk);
  for (int t = 0; t <= steps; ++t) {
    const int off = (t + 1) >> 1;
    const int chunk = (t & 1) ? own_chunk + off : own_chunk - off;
    if (chunk < 0 || chunk >= chunks) continue;
    // candidates: the block's box against the wave's box and the wave's largest K-th best (each lane one block)
    const float reach = wave_all(active ? best.d[K - 1] : -INFINITY, KnnMax());
    const int b = chunk * WAVE + lane_id();
    bool candidate = false;
    if (b < blocks && b != own) {
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
      const int count = min(KNN_BLOCK, n - blk * KNN_BLOCK);
      knn_scan<K>(best, rows + (int64_t)blk * KNN_BLOCK, count, q, self);
      scanned += (unsigned long long)lanes;
      evaluated += (unsigned long long)lanes * (unsigned long long)count;
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
  if (stats != nullptr && lane_id() == 0) {        // lane 0 of a wave that got here is active
    atomicAdd(stats + 0, scanned);
    atomicAdd(stats + 1, evaluated);
  }
}

template <int K>
static void knn_search_launch(const float4* rows, const float4* lo, const float4* hi, int n, int blocks, float* out_dist2,
                              int32_t* out_index, int64_t* out_stats, hipStream_t stream) {
  knn_search_kernel<K><<<(unsigned)blocks, KNN_BLOCK, 0, stream>>>(rows, lo, hi, n, blocks, out_dist2, out_index,
                                                                   (unsigned long long*)out_stats);
}

}  // namespace ms

using namespace ms;

extern "C" int ms_knn_points(const float* points3, const int32_t* order, int64_t n, int k, float* out_dist2,
                             int32_t* out_index, int64_t* out_stats, void* tmp, size_t* tmp_bytes, void* stream) {
  MS_CHECK_ARG(n >= 0, "n < 0");
  MS_CHECK_ARG(n < ((int64_t)1 << 31), "n >= 2^31 (indices are int32)");
  MS_CHECK_ARG(k >= 1 && k <= 8, "k must be in 1..8");
  const KnnScratch s = knn_scratch(n);
  MS_CHECK_TMP_AS(tmp, tmp_bytes, s.total, MS_ERR_BAD_ARG);   // this entry point's documented code for a short block
  if (n == 0) return 0;
  MS_CHECK_ARG(points3 != nullptr, "points3 is null");
  MS_CHECK_ARG(order != nullptr, "order is null");
  MS_CHECK_ARG(out_dist2 != nullptr, "out_dist2 is null");

  float4* rows = at<float4>(tmp, s.rows);
  float4* lo = at<float4>(tmp, s.lo);
  float4* hi = at<float4>(tmp, s.hi);
  const int blocks = (int)div_up(n, KNN_BLOCK);
  hipStream_t st = (hipStream_t)stream;
  knn_gather_blocks_kernel<<<(unsigned)blocks, KNN_BLOCK, 0, st>>>(points3, order, (int)n, rows, lo, hi);
  MS_CHECK_LAUNCH();
  switch (k) {
    case 1: knn_search_launch<1>(rows, lo, hi, (int)n, blocks, out_dist2, out_index, out_stats, st); break;
    case 2: knn_search_launch<2>(rows, lo, hi, (int)n, blocks, out_dist2, out_index, out_stats, st); break;
    case 3: knn_search_launch<3>(rows, lo, hi, (int)n, blocks, out_dist2, out_index, out_stats, st); break;
    case 4: knn_search_launch<4>(rows, lo, hi, (int)n, blocks, out_dist2, out_index, out_stats, st); break;
    case 5: knn_search_launch<5>(rows, lo, hi, (int)n, blocks, out_dist2, out_index, out_stats, st); break;
    case 6: knn_search_launch<6>(rows, lo, hi, (int)n, blocks, out_dist2, out_index, out_stats, st); break;
    case 7: knn_search_launch<7>(rows, lo, hi, (int)n, blocks, out_dist2, out_index, out_stats, st); break;
    default: knn_search_launch<8>(rows, lo, hi, (int)n, blocks, out_dist2, out_index, out_stats, st); break;
  }
  MS_CHECK_LAUNCH();
  return 0;
}
