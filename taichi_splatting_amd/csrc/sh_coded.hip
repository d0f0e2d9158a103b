// sh_coded.hip — view-dependent colour of a vector-quantised scene straight from its stored form (scene_codec.py; no
// reference counterpart): colour_c(i) = clamp(0.5 + Y_0 dc[i, c] + sum_{d >= 1} Y_d(dir_i) codebook[index[i], c, d - 1], 0, 1),
// float32, 3 channels, stored degree 1..3 (M = 3 / 8 / 15 codebook coefficients per channel).  Nothing is decoded.
//
// Forward (ms_sh_coded_fwd): one lane per gaussian in storage order; the code row (3 M floats, 4-byte aligned) is
// gathered as it is, 4 bytes at a time: the K rows live in L2.  (Gathering 16-byte pieces of a padded (K, 3, 16) copy
// was slower at degree 3, 0.227 ms against 0.192 at 6 M gaussians from a cold Infinity Cache: profiles/sh_coded.txt.)
// The products are summed in the order of sh_fwd_body (sh.hip): d = 0 .. D - 1, then + 0.5, then the clamp.
//
// Backward (ms_sh_coded_bwd): g = g_out where 0 < out < 1 (the strict-inside convention of sh_bwd_body), else 0.
//   sh_coded_prep_kernel      storage order: g_dc[i] = g Y_0, dense; with RECORDS also the 24-byte record (g, dir_i) of
//                             the gaussian into its slot of the code order, so that the next kernel reads whole lines
//                             (gathering position, out and g_out through the order instead took 0.80 ms where the two
//                             passes take 0.33 at 6 M gaussians: profiles/sh_coded.txt).
//   sh_coded_partial_kernel   one workgroup per chunk of MS_SH_CODED_CHUNK records (a chunk never spans two codes):
//                             lane = record evaluates the basis into LDS, then lane = (channel, coefficient) sums
//                             (double)g (double)Y over the records — wave w takes records w, w + 4, .. of each tile of
//                             256, the four sums combine as (0 + 1) + (2 + 3).
//   sh_coded_finish_kernel    one wave per code, lane = (channel, coefficient): the code's chunks in list order, rounded
//                             to float32 once.  A code without members gets zeros: every row is written.
// No atomics anywhere; the order of every sum is fixed by the plan, which depends on the index alone (the scheme of
// ms_kmeans_update, kmeans.hip).  The plan itself is built by the caller (spherical_harmonics.make_coded_sh_plan).
#include "common.h"

namespace ms {

constexpr int SC_THREADS = 256;
constexpr int SC_CHUNK = MS_SH_CODED_CHUNK;      // entries of the code order one workgroup sums
constexpr int SC_RECORD = 6;                     // floats of a record: the masked colour gradient, the unit direction
constexpr int SC_MAX_K = 65536;
static_assert(SC_CHUNK % SC_THREADS == 0, "a chunk is whole tiles of one entry per thread");

__device__ __forceinline__ int sc_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ void sc_direction(const float* __restrict__ positions, int64_t i3, const float* __restrict__ cam_pos,
                                             float& x, float& y, float& z) {
  const float dx = positions[i3 + 0] - cam_pos[0];
  const float dy = positions[i3 + 1] - cam_pos[1];
  const float dz = positions[i3 + 2] - cam_pos[2];
  const float len = t_sqrt(dx * dx + dy * dy + dz * dz);
  x = dx / len; y = dy / len; z = dz / len;
}

template <int DEG>
__global__ void __launch_bounds__(SC_THREADS)
sh_coded_fwd_kernel(const float* __restrict__ dc, const int32_t* __restrict__ index, const float* __restrict__ codebook,
                    const float* __restrict__ positions, const float* __restrict__ cam_pos, int n, int k_codes,
                    float* __restrict__ out) {
  constexpr int D = (DEG + 1) * (DEG + 1), M = D - 1;
  const int i = (int)blockIdx.x * SC_THREADS + (int)threadIdx.x;
  if (i >= n) return;
  const int64_t i3 = (int64_t)i * 3;
  float x, y, z;
  sc_direction(positions, i3, cam_pos, x, y, z);
  float Y[D];
  sh_basis<float, DEG>(x, y, z, Y);
  const int j = sc_clamp(index[i], 0, k_codes - 1);      // in 0..K-1 by contract; clamped so no access strays
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float acc = 0.0f;
    acc += Y[0] * dc[i3 + c];
    const float* row = codebook + ((int64_t)j * 3 + c) * M;
#pragma unroll
    for (int d = 1; d < D; ++d) acc += Y[d] * row[d - 1];
    out[i3 + c] = t_clamp(acc + 0.5f, 0.0f, 1.0f);
  }
}

template <bool RECORDS>
__global__ void __launch_bounds__(SC_THREADS)
sh_coded_prep_kernel(const float* __restrict__ positions, const float* __restrict__ cam_pos, const float* __restrict__ out,
                     const float* __restrict__ g_out, const int32_t* __restrict__ rank, int n, float* __restrict__ g_dc,
                     float* __restrict__ records) {
  const int i = (int)blockIdx.x * SC_THREADS + (int)threadIdx.x;
  if (i >= n) return;
  const int64_t i3 = (int64_t)i * 3;
  float g[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float o = out[i3 + c];
    g[c] = (o > 0.0f && o < 1.0f) ? g_out[i3 + c] : 0.0f;
  }
  if (g_dc != nullptr) {
#pragma unroll
    for (int c = 0; c < 3; ++c) g_dc[i3 + c] = g[c] * float(MS_SH_C0);
  }
  if constexpr (RECORDS) {
    float x, y, z;
    sc_direction(positions, i3, cam_pos, x, y, z);
    float2* rec = reinterpret_cast<float2*>(records + (int64_t)sc_clamp(rank[i], 0, n - 1) * SC_RECORD);
    rec[0] = make_float2(g[0], g[1]);
    rec[1] = make_float2(g[2], x);
    rec[2] = make_float2(y, z);
  }
}

template <int DEG>
__global__ void __launch_bounds__(SC_THREADS)
sh_coded_partial_kernel(const float* __restrict__ records, const int32_t* __restrict__ chunk_begin, int num_chunks, int n,
                        double* __restrict__ partial) {
  constexpr int D = (DEG + 1) * (DEG + 1), M = D - 1, ROW = 3 * M, YS = M | 1, WAVES = SC_THREADS / WAVE;
  static_assert(ROW <= WAVE, "one lane per (channel, coefficient)");
  __shared__ float s_Y[SC_THREADS * YS];      // odd row stride: the writes of a wave's 64 entries miss each other's banks
  __shared__ float s_g[SC_THREADS * 3];
  __shared__ double s_sum[WAVES][ROW];

  const int chunk = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // a chunk ends where the next one begins (chunks cover the code order without gaps) and never holds more than SC_CHUNK
  const int begin = sc_clamp(chunk_begin[chunk], 0, n);
  const int next = chunk + 1 < num_chunks ? sc_clamp(chunk_begin[chunk + 1], 0, n) : n;
  const int end = min(next, begin + SC_CHUNK);
  const int c = lane / M, d = lane - c * M;

  double acc = 0.0;
  for (int t0 = begin; t0 < end; t0 += SC_THREADS) {
    const int e = t0 + tid;
    if (e < end) {
      const float2* rec = reinterpret_cast<const float2*>(records + (int64_t)e * SC_RECORD);
      const float2 r0 = rec[0], r1 = rec[1], r2 = rec[2];
      const float g[3] = {r0.x, r0.y, r1.x};
      float Y[D];
      sh_basis<float, DEG>(r1.y, r2.x, r2.y, Y);
#pragma unroll
      for (int q = 0; q < M; ++q) s_Y[tid * YS + q] = Y[q + 1];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) s_g[tid * 3 + ch] = g[ch];
    }
    __syncthreads();
    const int count = min(SC_THREADS, end - t0);
    if (lane < ROW)
      for (int q = wave; q < count; q += WAVES) acc += (double)s_g[q * 3 + c] * (double)s_Y[q * YS + d];
    __syncthreads();                                   // the tile has been consumed
  }
  if (lane < ROW) s_sum[wave][lane] = acc;
  __syncthreads();
  if (tid < ROW) partial[(int64_t)chunk * ROW + tid] = (s_sum[0][tid] + s_sum[1][tid]) + (s_sum[2][tid] + s_sum[3][tid]);
}

// One wave per code, four codes per workgroup.  chunk_off[j] .. chunk_off[j + 1] are the chunks of code j.
__global__ void __launch_bounds__(SC_THREADS)
sh_coded_finish_kernel(const double* __restrict__ partial, const int32_t* __restrict__ chunk_off, int num_chunks, int k_codes,
                       int row, float* __restrict__ g_codebook) {
  const int code = (int)blockIdx.x * (SC_THREADS / WAVE) + ((int)threadIdx.x >> 6), lane = lane_id();
  if (code >= k_codes || lane >= row) return;
  const int c0 = sc_clamp(chunk_off[code], 0, num_chunks), c1 = sc_clamp(chunk_off[code + 1], c0, num_chunks);
  double s = 0.0;
  for (int ch = c0; ch < c1; ++ch) s += partial[(int64_t)ch * row + lane];
  g_codebook[(int64_t)code * row + lane] = (float)s;
}

struct ShCodedScratch {
  size_t partial, records, total;
};

static ShCodedScratch sh_coded_scratch(int64_t n, int64_t num_chunks, int degree) {
  const size_t row = 3 * (size_t)((degree + 1) * (degree + 1) - 1);
  Carve c;
  ShCodedScratch s;
  s.partial = c.take((size_t)(num_chunks > 0 ? num_chunks : 1) * row * sizeof(double));
  s.records = c.take((size_t)n * SC_RECORD * sizeof(float));
  s.total = c.off;
  return s;
}

}  // namespace ms

using namespace ms;

#define SH_CODED_CHECK_SHAPE()                                                              \
  MS_CHECK_ARG(n >= 0, "n < 0");                                                            \
  MS_CHECK_ARG(n < ((int64_t)1 << 31) - SC_CHUNK, "n >= 2^31 - 512 (the code order is int32)"); \
  MS_CHECK_ARG(sh_degree >= 1 && sh_degree <= 3, "sh_degree must be in 1..3");              \
  MS_CHECK_ARG(k >= 1 && k <= SC_MAX_K, "k must be in 1..65536")

extern "C" int ms_sh_coded_fwd(const float* dc, const int32_t* index, const float* codebook, const float* positions,
                               const float* cam_pos, int64_t n, int k, int sh_degree, float* out, void* stream) {
  SH_CODED_CHECK_SHAPE();
  if (n == 0) return 0;
  MS_CHECK_ARG(dc != nullptr, "dc is null");
  MS_CHECK_ARG(index != nullptr, "index is null");
  MS_CHECK_ARG(codebook != nullptr, "codebook is null");
  MS_CHECK_ARG(positions != nullptr, "positions is null");
  MS_CHECK_ARG(cam_pos != nullptr, "cam_pos is null");
  MS_CHECK_ARG(out != nullptr, "out is null");

  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)div_up(n, SC_THREADS)), block(SC_THREADS);
#define MS_SH_CODED_FWD(DEG) \
  sh_coded_fwd_kernel<DEG><<<grid, block, 0, st>>>(dc, index, codebook, positions, cam_pos, (int)n, k, out)
  switch (sh_degree) {
    case 1: MS_SH_CODED_FWD(1); break;
    case 2: MS_SH_CODED_FWD(2); break;
    default: MS_SH_CODED_FWD(3); break;
  }
#undef MS_SH_CODED_FWD
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_sh_coded_bwd(const float* positions, const float* cam_pos, const float* out, const float* g_out,
                               const int32_t* rank, const int32_t* chunk_begin, const int32_t* chunk_off,
                               int64_t num_chunks, int64_t n, int k, int sh_degree, float* g_dc, float* g_codebook, void* tmp,
                               size_t* tmp_bytes, void* stream) {
  SH_CODED_CHECK_SHAPE();
  MS_CHECK_ARG(num_chunks >= 0 && num_chunks <= n, "num_chunks must be in 0..n (a chunk holds at least one entry)");
  const ShCodedScratch s = sh_coded_scratch(n, num_chunks, sh_degree);
  MS_CHECK_TMP(tmp, tmp_bytes, s.total);
  if (g_dc == nullptr && g_codebook == nullptr) return 0;

  hipStream_t st = (hipStream_t)stream;
  const int row = 3 * ((sh_degree + 1) * (sh_degree + 1) - 1);
  if (n == 0) {                                            // every code is empty
    if (g_codebook != nullptr) MS_CHECK_HIP(hipMemsetAsync(g_codebook, 0, (size_t)k * row * sizeof(float), st));
    return 0;
  }
  MS_CHECK_ARG(out != nullptr, "out is null");
  MS_CHECK_ARG(g_out != nullptr, "g_out is null");
  if (g_codebook != nullptr) {
    MS_CHECK_ARG(positions != nullptr, "positions is null");
    MS_CHECK_ARG(cam_pos != nullptr, "cam_pos is null");
    MS_CHECK_ARG(chunk_begin != nullptr || num_chunks == 0, "chunk_begin is null");
    MS_CHECK_ARG(chunk_off != nullptr, "chunk_off is null");
    MS_CHECK_ARG(rank != nullptr, "rank is null");
  }

  double* partial = at<double>(tmp, s.partial);
  float* recs = at<float>(tmp, s.records);
  const dim3 block(SC_THREADS), point_grid((unsigned)div_up(n, SC_THREADS));
  if (g_codebook != nullptr) {
    sh_coded_prep_kernel<true><<<point_grid, block, 0, st>>>(positions, cam_pos, out, g_out, rank, (int)n, g_dc, recs);
    MS_CHECK_LAUNCH();
  } else if (g_dc != nullptr) {
    sh_coded_prep_kernel<false><<<point_grid, block, 0, st>>>(nullptr, nullptr, out, g_out, nullptr, (int)n, g_dc, nullptr);
    MS_CHECK_LAUNCH();
  }
  if (g_codebook == nullptr) return 0;
  if (num_chunks > 0) {
    const dim3 grid((unsigned)num_chunks);
#define MS_SH_CODED_PARTIAL(DEG) \
  sh_coded_partial_kernel<DEG><<<grid, block, 0, st>>>(recs, chunk_begin, (int)num_chunks, (int)n, partial)
    switch (sh_degree) {
      case 1: MS_SH_CODED_PARTIAL(1); break;
      case 2: MS_SH_CODED_PARTIAL(2); break;
      default: MS_SH_CODED_PARTIAL(3); break;
    }
#undef MS_SH_CODED_PARTIAL
    MS_CHECK_LAUNCH();
  }
  sh_coded_finish_kernel<<<dim3((unsigned)div_up(k, SC_THREADS / WAVE)), block, 0, st>>>(partial, chunk_off, (int)num_chunks, k, row,
                                                                                         g_codebook);
  MS_CHECK_LAUNCH();
  return 0;
}
