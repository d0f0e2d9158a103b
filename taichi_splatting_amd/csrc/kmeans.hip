// kmeans.hip — the two halves of a Lloyd iteration over N points of dimension D <= 64 and K <= 65 536 codes: what
// scene_codec.py vector-quantises the SH coefficients of a scene with (no reference counterpart).
//
// Assignment (ms_kmeans_assign) is a GEMM with an arg-min epilogue on the exact f32-input MFMA v_mfma_f32_32x32x2_f32:
//
//   kmeans_codes_kernel        the codebook into the image a workgroup stages: zero-padded to DP = D rounded up to 8 and
//                              K rounded up to KM_CHUNK, permuted so that the B fragments of four k-steps are one 16-byte
//                              LDS read; and ||c_j||^2 (float64 sum, rounded once; +inf for a padded code).
//   kmeans_assign_kernel<DP>   256 threads own 256 points, each wave KM_MT tiles of 32.  A = -2 x (a lane keeps its
//                              row's DP/2 values per tile in registers for the whole kernel), B = a tile of 32 codes from
//                              LDS, C = ||c_j||^2 of the lane's column, so the accumulator IS the score
//                              s(i, j) = ||c_j||^2 - 2 x_i.c_j.  Per accumulator register a running (best score, tile)
//                              with strict <; one lexicographic (score, index) butterfly over the 32 lanes of a point's
//                              columns at the end.  KM_CHUNK codes are staged per pass, by a straight 16-byte copy.
//
// Lane maps (32x32x2): A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31], C/D register r of a lane is
// column lane & 31, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  MFMA step s of a tile multiplies k = 2 s + (lane >> 5).
//
// Update (ms_kmeans_update) is reproducible by construction: the (code, point) pairs are sorted by code with the stable
// ms_radix_sort_pairs, so a code's members are a run in ascending point order; a run is cut into chunks of
// KM_UPDATE_CHUNK entries; a workgroup sums one chunk in float64 in a fixed order (wave w takes entries w, w + 4, ...,
// the four partial sums combine as (0 + 1) + (2 + 3)); one lane per (code, dimension) adds the code's chunks in list
// order and divides.  No atomics anywhere.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace ms {

constexpr int KM_THREADS = 256;
constexpr int KM_MT = 2;                                   // 32-point tiles a wave keeps in flight
constexpr int KM_TILE = 32;                                // codes of one MFMA tile
constexpr int KM_WAVE_POINTS = KM_TILE * KM_MT;
constexpr int KM_POINTS = (KM_THREADS / WAVE) * KM_WAVE_POINTS;     // points of a workgroup
constexpr int KM_CHUNK = MS_KMEANS_CHUNK;                  // codes staged per pass
constexpr int KM_CHUNK_TILES = KM_CHUNK / KM_TILE;
constexpr int KM_UPDATE_CHUNK = MS_KMEANS_UPDATE_CHUNK;    // sorted entries one workgroup of the update sums
constexpr int KM_MAX_D = MS_KMEANS_MAX_D, KM_MAX_K = MS_KMEANS_MAX_K;
static_assert(KM_POINTS == 256 && KM_CHUNK % KM_TILE == 0 && KM_MAX_D == 64, "kmeans tiling");

typedef float f32x16 __attribute__((ext_vector_type(16)));

static inline int kmeans_padded_d(int d) { return (d + 7) / 8 * 8; }
static inline int64_t kmeans_padded_k(int k) { return div_up(k, KM_CHUNK) * KM_CHUNK; }

// ---- assignment ------------------------------------------------------------------------------------------------

// One thread per 16 bytes of the staged image.  Tile T (32 codes) is DP / 8 groups g x 2 halves h x 32 columns j of
// float4; element q of that float4 is c[32 T + j][k = 8 g + 2 q + h]: what lane (j, h) multiplies in MFMA steps
// 4 g .. 4 g + 3.  The threads of (g, h) = (0, 0) also write the norm of their code.
__global__ void __launch_bounds__(KM_THREADS)
kmeans_codes_kernel(const float* __restrict__ codebook, int k_codes, int d, int dp, int64_t k_padded,
                    float4* __restrict__ packed, float* __restrict__ norms) {
  const int64_t t = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x;
  const int per_tile = dp * 8;                           // float4 of one tile
  if (t >= k_padded / KM_TILE * per_tile) return;
  const int64_t tile = t / per_tile;
  const int f = (int)(t - tile * per_tile);
  const int j = f & 31, h = (f >> 5) & 1, g = f >> 6;
  const int64_t code = tile * KM_TILE + j;
  const bool real = code < k_codes;
  float v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = 8 * g + 2 * q + h;
    v[q] = (real && k < d) ? codebook[code * d + k] : 0.0f;
  }
  packed[t] = make_float4(v[0], v[1], v[2], v[3]);
  if (g == 0 && h == 0) {
    double s = 0.0;
    if (real)
      for (int k = 0; k < d; ++k) {
        const double c = (double)codebook[code * d + k];
        s += c * c;
      }
    norms[code] = real ? (float)s : INFINITY;
  }
}

template <int DP>
__global__ void __launch_bounds__(KM_THREADS)
kmeans_assign_kernel(const float* __restrict__ x, int n, int d, const float4* __restrict__ packed,
                     const float* __restrict__ norms, int k_codes, int32_t* __restrict__ out_index,
                     float* __restrict__ out_dist2) {
  constexpr int STEPS = DP / 2, GROUPS = DP / 8, TILE_F4 = DP * 8, CHUNK_F4 = KM_CHUNK_TILES * TILE_F4;
  __shared__ float4 lds_codes[CHUNK_F4];
  __shared__ float lds_norm[KM_CHUNK];

  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const int base = (int)blockIdx.x * KM_POINTS + wave * KM_WAVE_POINTS;

  // A fragments: -2 x (exact), zero past D and past N
  float a[KM_MT][STEPS];
#pragma unroll
  for (int mt = 0; mt < KM_MT; ++mt) {
    const int row = base + mt * KM_TILE + col;
    const float* xr = x + (int64_t)min(row, n - 1) * d;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      const int k = 2 * s + half;
      a[mt][s] = (row < n && k < d) ? -2.0f * xr[k] : 0.0f;
    }
  }

  f32x16 best[KM_MT];
  int best_tile[KM_MT][16];
#pragma unroll
  for (int mt = 0; mt < KM_MT; ++mt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      best[mt][r] = INFINITY;
      best_tile[mt][r] = 0;
    }
  }

  const int chunks = (k_codes + KM_CHUNK - 1) / KM_CHUNK;
  for (int c = 0; c < chunks; ++c) {
    __syncthreads();                                     // the previous chunk has been consumed
    const float4* src = packed + (int64_t)c * CHUNK_F4;
#pragma unroll
    for (int i = 0; i < CHUNK_F4 / KM_THREADS; ++i) lds_codes[i * KM_THREADS + tid] = src[i * KM_THREADS + tid];
    if (tid < KM_CHUNK) lds_norm[tid] = norms[(int64_t)c * KM_CHUNK + tid];
    __syncthreads();

    const int tiles = min(KM_CHUNK_TILES, (k_codes - c * KM_CHUNK + KM_TILE - 1) / KM_TILE);
    for (int t = 0; t < tiles; ++t) {
      const float cn = lds_norm[t * KM_TILE + col];
      f32x16 acc[KM_MT];
#pragma unroll
      for (int mt = 0; mt < KM_MT; ++mt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = cn;
      }
#pragma unroll
      for (int g = 0; g < GROUPS; ++g) {
        const float4 b = lds_codes[t * TILE_F4 + (g * 2 + half) * 32 + col];
        const float bq[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
          for (int mt = 0; mt < KM_MT; ++mt)
            acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt][4 * g + q], bq[q], acc[mt], 0, 0, 0);
        }
      }
      const int tile_id = c * KM_CHUNK_TILES + t;
#pragma unroll
      for (int mt = 0; mt < KM_MT; ++mt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const bool better = acc[mt][r] < best[mt][r];        // strict: the earlier tile keeps a tie
          best[mt][r] = better ? acc[mt][r] : best[mt][r];
          best_tile[mt][r] = better ? tile_id : best_tile[mt][r];
        }
      }
    }
  }

  // one (score, index) minimum per point over the 32 lanes of its columns; lane col == r keeps register r's
#pragma unroll
  for (int mt = 0; mt < KM_MT; ++mt) {
    float keep_v = 0.0f;
    int keep_id = 0, keep_row = n;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v = best[mt][r];
      int id = best_tile[mt][r] * KM_TILE + col;
#pragma unroll
      for (int off = 16; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int oid = __shfl_xor(id, off, 64);
        const bool take = ov < v || (ov == v && oid < id);
        v = take ? ov : v;
        id = take ? oid : id;
      }
      if (col == r) {
        keep_v = v;
        keep_id = id;
        keep_row = base + mt * KM_TILE + (r & 3) + 8 * (r >> 2) + 4 * half;
      }
    }
    if (col < 16 && keep_row < n) {
      out_index[keep_row] = min(keep_id, k_codes - 1);   // a NaN score never wins and leaves 0; never past K
      if (out_dist2 != nullptr) {
        const float* xr = x + (int64_t)keep_row * d;
        double s = 0.0;
        for (int k = 0; k < d; ++k) {
          const double xv = (double)xr[k];
          s += xv * xv;
        }
        out_dist2[keep_row] = fmaxf(keep_v + (float)s, 0.0f);
      }
    }
  }
}

template <int DP>
static void kmeans_assign_launch(const float* x, int n, int d, const float4* packed, const float* norms, int k,
                                 int32_t* out_index, float* out_dist2, hipStream_t st) {
  kmeans_assign_kernel<DP><<<(unsigned)div_up(n, KM_POINTS), KM_THREADS, 0, st>>>(x, n, d, packed, norms, k, out_index, out_dist2);
}

struct KMeansAssignScratch {
  size_t packed, norms, total;
};

static KMeansAssignScratch kmeans_assign_scratch(int d, int k) {
  const size_t kp = (size_t)kmeans_padded_k(k);
  Carve c;
  KMeansAssignScratch s;
  s.packed = c.take(kp * (size_t)kmeans_padded_d(d) * sizeof(float));
  s.norms = c.take(kp * sizeof(float));
  s.total = c.off;
  return s;
}

// ---- update ----------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(KM_THREADS)
kmeans_pairs_kernel(const int32_t* __restrict__ index, int n, int k_codes, uint32_t* __restrict__ keys,
                    int32_t* __restrict__ vals) {
  const int i = (int)blockIdx.x * KM_THREADS + (int)threadIdx.x;
  if (i >= n) return;
  keys[i] = (uint32_t)min(max(index[i], 0), k_codes - 1);   // in 0..K-1 by contract; clamped so no access strays
  vals[i] = i;
}

// start[c] = first sorted entry whose code is >= c, for c in 0..K: the entry that opens a run writes the starts of its
// own code and of the empty codes before it, the last entry those after it.  Every start is written exactly once.
__global__ void __launch_bounds__(KM_THREADS)
kmeans_ranges_kernel(const uint32_t* __restrict__ sorted_keys, int n, int k_codes, int32_t* __restrict__ start) {
  const int i = (int)blockIdx.x * KM_THREADS + (int)threadIdx.x;
  if (i >= n) return;
  const int key = min((int)sorted_keys[i], k_codes - 1);
  const int prev = i > 0 ? min((int)sorted_keys[i - 1], k_codes - 1) : -1;
  for (int c = prev + 1; c <= key; ++c) start[c] = i;
  if (i == n - 1)
    for (int c = key + 1; c <= k_codes; ++c) start[c] = n;
}

constexpr int KM_SCAN_THREADS = 1024;

// chunk_off[j] = chunks of the codes before j (exclusive scan of ceil(members / KM_UPDATE_CHUNK)), chunk_off[K] = total
__global__ void __launch_bounds__(KM_SCAN_THREADS)
kmeans_chunk_scan_kernel(const int32_t* __restrict__ start, int k_codes, int32_t* __restrict__ chunk_off) {
  __shared__ int part[KM_SCAN_THREADS];
  const int tid = (int)threadIdx.x;
  const int per = (k_codes + KM_SCAN_THREADS - 1) / KM_SCAN_THREADS;
  const int lo = min(tid * per, k_codes), hi = min(lo + per, k_codes);
  int sum = 0;
  for (int j = lo; j < hi; ++j) sum += (start[j + 1] - start[j] + KM_UPDATE_CHUNK - 1) / KM_UPDATE_CHUNK;
  part[tid] = sum;
  __syncthreads();
  for (int off = 1; off < KM_SCAN_THREADS; off <<= 1) {
    const int v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int run = part[tid] - sum;
  for (int j = lo; j < hi; ++j) {
    chunk_off[j] = run;
    run += (start[j + 1] - start[j] + KM_UPDATE_CHUNK - 1) / KM_UPDATE_CHUNK;
  }
  if (tid == KM_SCAN_THREADS - 1) chunk_off[k_codes] = part[tid];
}

// One workgroup per chunk: lane = dimension, the four waves stride the chunk's entries.  partial[chunk][0..D) are the
// weighted sums, partial[chunk][D] the weight sum.
__global__ void __launch_bounds__(KM_THREADS)
kmeans_partial_kernel(const float* __restrict__ x, const float* __restrict__ weights, const int32_t* __restrict__ sorted_vals,
                      const int32_t* __restrict__ start, const int32_t* __restrict__ chunk_off, int n, int k_codes, int d,
                      double* __restrict__ partial) {
  __shared__ double sums[KM_THREADS / WAVE][KM_MAX_D + 1];
  const int chunk = (int)blockIdx.x;
  if (chunk >= chunk_off[k_codes]) return;               // uniform over the workgroup
  int lo = 0, hi = k_codes;                              // first code whose chunk_off is past this chunk
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (chunk_off[mid] > chunk) hi = mid; else lo = mid + 1;
  }
  const int code = max(lo - 1, 0);
  const int begin = start[code] + (chunk - chunk_off[code]) * KM_UPDATE_CHUNK;
  const int end = min(min(begin + KM_UPDATE_CHUNK, start[code + 1]), n);

  const int lane = lane_id(), wave = (int)threadIdx.x >> 6;
  constexpr int WAVES = KM_THREADS / WAVE;
  double acc = 0.0, wacc = 0.0;
  for (int e = begin + wave; e < end; e += WAVES) {
    const int p = min(max(sorted_vals[e], 0), n - 1);
    const float w = weights != nullptr ? weights[p] : 1.0f;
    if (lane < d) acc += (double)w * (double)x[(int64_t)p * d + lane];
    wacc += (double)w;
  }
  sums[wave][lane] = acc;
  if (lane == 0) sums[wave][KM_MAX_D] = wacc;
  __syncthreads();
  const int t = (int)threadIdx.x;
  if (t <= d) {
    const int slot = t < d ? t : KM_MAX_D;
    partial[(int64_t)chunk * (d + 1) + t] = (sums[0][slot] + sums[1][slot]) + (sums[2][slot] + sums[3][slot]);
  }
}

// One wave per code, lane = dimension: the code's chunks in list order.  A code without members or without weight keeps
// its centroid (nothing is stored to it).
__global__ void __launch_bounds__(WAVE)
kmeans_finish_kernel(const double* __restrict__ partial, const int32_t* __restrict__ start, const int32_t* __restrict__ chunk_off,
                     int d, float* __restrict__ codebook, int32_t* __restrict__ counts, double* __restrict__ weight_sums) {
  const int code = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int count = start[code + 1] - start[code];
  const int c0 = chunk_off[code], c1 = chunk_off[code + 1];
  double s = 0.0, w = 0.0;
  for (int c = c0; c < c1; ++c) {
    if (lane < d) s += partial[(int64_t)c * (d + 1) + lane];
    w += partial[(int64_t)c * (d + 1) + d];
  }
  if (lane < d && count > 0 && w > 0.0) codebook[(int64_t)code * d + lane] = (float)(s / w);
  if (lane == 0) {
    counts[code] = count;
    if (weight_sums != nullptr) weight_sums[code] = w;
  }
}

struct KMeansUpdateScratch {
  size_t keys_in, vals_in, keys_out, vals_out, start, chunk_off, partial, sort, sort_bytes, total;
};

static KMeansUpdateScratch kmeans_update_scratch(int64_t n, int d, int k) {
  const size_t pairs = (size_t)n * 4, offs = ((size_t)k + 1) * 4;
  const size_t max_chunks = (size_t)div_up(n, KM_UPDATE_CHUNK) + (size_t)k;
  Carve c;
  KMeansUpdateScratch s;
  s.keys_in = c.take(pairs);
  s.vals_in = c.take(pairs);
  s.keys_out = c.take(pairs);
  s.vals_out = c.take(pairs);
  s.start = c.take(offs);
  s.chunk_off = c.take(offs);
  s.partial = c.take(max_chunks * (size_t)(d + 1) * sizeof(double));
  s.sort_bytes = sort_tmp_size(n, 4);
  s.sort = c.take(s.sort_bytes);
  s.total = c.off;
  return s;
}

}  // namespace ms

using namespace ms;

#define KMEANS_CHECK_SHAPE()                                                              \
  MS_CHECK_ARG(n >= 0, "n < 0");                                                          \
  MS_CHECK_ARG(n < ((int64_t)1 << 31) - KM_UPDATE_CHUNK, "n >= 2^31 - 1024 (indices are int32)"); \
  MS_CHECK_ARG(d >= 1 && d <= KM_MAX_D, "d must be in 1..64");                            \
  MS_CHECK_ARG(k >= 1 && k <= KM_MAX_K, "k must be in 1..65536")

extern "C" int ms_kmeans_assign(const float* x, int64_t n, int d, const float* codebook, int k, int32_t* out_index,
                                float* out_dist2, void* tmp, size_t* tmp_bytes, void* stream) {
  KMEANS_CHECK_SHAPE();
  const KMeansAssignScratch s = kmeans_assign_scratch(d, k);
  MS_CHECK_TMP(tmp, tmp_bytes, s.total);
  if (n == 0) return 0;
  MS_CHECK_ARG(x != nullptr, "x is null");
  MS_CHECK_ARG(codebook != nullptr, "codebook is null");
  MS_CHECK_ARG(out_index != nullptr, "out_index is null");

  float4* packed = at<float4>(tmp, s.packed);
  float* norms = at<float>(tmp, s.norms);
  hipStream_t st = (hipStream_t)stream;
  const int dp = kmeans_padded_d(d);
  const int64_t kp = kmeans_padded_k(k);
  kmeans_codes_kernel<<<(unsigned)div_up(kp * dp / 4, KM_THREADS), KM_THREADS, 0, st>>>(codebook, k, d, dp, kp, packed, norms);
  MS_CHECK_LAUNCH();
  switch (dp) {
    case 8: kmeans_assign_launch<8>(x, (int)n, d, packed, norms, k, out_index, out_dist2, st); break;
    case 16: kmeans_assign_launch<16>(x, (int)n, d, packed, norms, k, out_index, out_dist2, st); break;
    case 24: kmeans_assign_launch<24>(x, (int)n, d, packed, norms, k, out_index, out_dist2, st); break;
    case 32: kmeans_assign_launch<32>(x, (int)n, d, packed, norms, k, out_index, out_dist2, st); break;
    case 40: kmeans_assign_launch<40>(x, (int)n, d, packed, norms, k, out_index, out_dist2, st); break;
    case 48: kmeans_assign_launch<48>(x, (int)n, d, packed, norms, k, out_index, out_dist2, st); break;
    case 56: kmeans_assign_launch<56>(x, (int)n, d, packed, norms, k, out_index, out_dist2, st); break;
    default: kmeans_assign_launch<64>(x, (int)n, d, packed, norms, k, out_index, out_dist2, st); break;
  }
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_kmeans_update(const float* x, const int32_t* index, const float* weights, int64_t n, int d, int k,
                                float* codebook, int32_t* out_counts, double* out_weight_sums, void* tmp,
                                size_t* tmp_bytes, void* stream) {
  KMEANS_CHECK_SHAPE();
  const KMeansUpdateScratch s = kmeans_update_scratch(n, d, k);
  MS_CHECK_TMP(tmp, tmp_bytes, s.total);
  MS_CHECK_ARG(codebook != nullptr, "codebook is null");
  MS_CHECK_ARG(out_counts != nullptr, "out_counts is null");
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {                                           // every code is empty: centroids stay
    MS_CHECK_HIP(hipMemsetAsync(out_counts, 0, (size_t)k * sizeof(int32_t), st));
    if (out_weight_sums != nullptr) MS_CHECK_HIP(hipMemsetAsync(out_weight_sums, 0, (size_t)k * sizeof(double), st));
    return 0;
  }
  MS_CHECK_ARG(x != nullptr, "x is null");
  MS_CHECK_ARG(index != nullptr, "index is null");

  uint32_t* keys_in = at<uint32_t>(tmp, s.keys_in);
  int32_t* vals_in = at<int32_t>(tmp, s.vals_in);
  uint32_t* keys_out = at<uint32_t>(tmp, s.keys_out);
  int32_t* vals_out = at<int32_t>(tmp, s.vals_out);
  int32_t* start = at<int32_t>(tmp, s.start);
  int32_t* chunk_off = at<int32_t>(tmp, s.chunk_off);
  double* partial = at<double>(tmp, s.partial);
  const unsigned point_blocks = (unsigned)div_up(n, KM_THREADS);

  kmeans_pairs_kernel<<<point_blocks, KM_THREADS, 0, st>>>(index, (int)n, k, keys_in, vals_in);
  MS_CHECK_LAUNCH();
  size_t sort_bytes = s.sort_bytes;
  const int sort_rc = ms_radix_sort_pairs(keys_in, vals_in, keys_out, vals_out, n, 4, 0, 16,
                                          at<char>(tmp, s.sort), &sort_bytes, stream);
  if (sort_rc != 0) return sort_rc;
  kmeans_ranges_kernel<<<point_blocks, KM_THREADS, 0, st>>>(keys_out, (int)n, k, start);
  MS_CHECK_LAUNCH();
  kmeans_chunk_scan_kernel<<<1, KM_SCAN_THREADS, 0, st>>>(start, k, chunk_off);
  MS_CHECK_LAUNCH();
  const unsigned max_chunks = (unsigned)(div_up(n, KM_UPDATE_CHUNK) + k);
  kmeans_partial_kernel<<<max_chunks, KM_THREADS, 0, st>>>(x, weights, vals_out, start, chunk_off, (int)n, k, d, partial);
  MS_CHECK_LAUNCH();
  kmeans_finish_kernel<<<(unsigned)k, WAVE, 0, st>>>(partial, start, chunk_off, d, codebook, out_counts, out_weight_sums);
  MS_CHECK_LAUNCH();
  return 0;
}
