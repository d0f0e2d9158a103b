// raster_wide.hip — single-pass alpha compositing of (V, F) float32 features, 1 <= F <= 128, on the existing tile lists,
// with its contractions on the exact f32-input MFMA v_mfma_f32_32x32x2_f32 (no reference counterpart: the reference and
// the generic templates of raster.hip render wide features four channels at a time, each chunk gathering the tile
// lists, evaluating every (pixel, splat) alpha and committing the geometry gradient again).
//
// Semantics are those of raster_fwd_kernel / raster_bwd_kernel<float, F, 16, AA = false, ...> with alpha blending
// (rasterizer/forward.py:39-135, rasterizer/backward.py:97-224): gate alpha > alpha_threshold after the clamp to
// clamp_max_alpha, front-to-back order of the tile's range, out-of-bounds pixels inert, image_weight = accumulated
// alpha, the backward drops a pair once the weight in front of it has reached saturate_threshold.
//
// Shared organisation: tile 16, one workgroup of 256 threads per tile, one wave per 8 x 8 patch, one lane per pixel for
// the alpha chain; the tile's list is staged WIDE_BATCH = 64 splats at a time (blend / cull records of raster_common.h,
// feature rows zero-padded to FP = 32 NB channels, NB = ceil(F / 32) a template parameter, rows FP + 1 floats apart so
// that both a row read (32 consecutive channels) and a column read (32 splats, one channel) are free of bank
// conflicts); every wave tests the batch against its patch with one splat per lane, ballots, and walks the hits.
//
// Forward: hits are consumed two at a time.  The lane of pixel l has the blend weights w0[l], w1[l] of the two splats
// (VALU, sequential transmittance chain); ONE v_permlane32_swap(w0, w1) yields the A operands of both 32-pixel row
// blocks (A[i = l & 31][k = l >> 5]); B is one LDS read per channel block (lanes 0-31 the first splat's 32 channels,
// lanes 32-63 the second's); 2 NB MFMAs accumulate into 2 NB 32 x 32 tiles.  An odd last hit pairs with weight 0.  In the
// C/D layout a lane holds one channel (column l & 31) and rows (r & 3) + 8 (r >> 2) + 4 (l >> 5), so a half-wave stores
// 32 consecutive channels of one pixel.  The MFMA is a k-ordered fmaf chain: every channel block sees the same chain
// whatever NB is, there are no atomics, and two runs are bitwise equal.
//
// Backward: with g[p][s] = sum_c G[p][c] f[s][c] the per-pixel state is scalar whatever F is:
//   dL/dalpha[p][s] = T g[p][s] - (G[p].C[p] - sum_{k <= s} w[p][k] g[p][k]) / (1 - alpha)
// (the 1-channel backward with the per-pixel "feature" g).  Hits are compacted per wave and taken 32 at a time:
//   1. g^T = feats . G^T (rows = 32 hits, columns = pixels, K = FP channels): A from the staged rows, B = the wave's G,
//      held in FP registers for the whole kernel; 16 v_permlane32_swap hand every lane the 32 values of ITS pixel;
//   2. the scalar chain per lane and the seven geometric sums, reduced per (patch, splat) with wave_reduce16 and
//      committed with one float atomic instruction, as the pixel-per-lane backward of raster_fast.hip does;
//   3. grad_feats = W^T . G (rows = 32 hits, columns = 32 channels, K = the wave's 64 pixels): the chain leaves its
//      weights in LDS transposed (A), B streams dL/dimage rows from L1 / L2 (a half-wave reads one pixel's 128
//      consecutive bytes); the four waves of the tile add their tiles into one LDS block per batch, which is committed
//      with one atomic per (tile, splat, channel).
// G of the tile does not fit in LDS next to the rest at F = 128 (132 KB), hence registers for 1 and the cache for 3.
// Either gradient may be absent (template parameter): without grad_points7 piece 1, the feature staging and the
// gradient part of the chain are gone (feature distillation on frozen geometry).
#include "raster_common.h"

namespace ms {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int WIDE_BATCH = 64;
constexpr int WIDE_THREADS = 256;

struct WideParams {
  int width, height, tiles_wide, f;
  float clamp_max_alpha, alpha_threshold, saturate_threshold;
};

// rows (splats in the backward, pixels in the forward) of accumulator register r in lane half h
__device__ __forceinline__ int mfma_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

template <int NB, bool FEATS>
__device__ __forceinline__ void wide_stage(const float* __restrict__ points, const float* __restrict__ feats,
                                           const int32_t* __restrict__ o2p, int begin, int count, int f,
                                           float alpha_threshold, float4* s_rec, float4* s_cull, int32_t* s_id,
                                           float* s_feat) {
  constexpr int FP = 32 * NB, FS = FP + 1;
  const int tid = threadIdx.x;
  if (tid < count) {
    const int32_t id = o2p[begin + tid];
    const float* g = points + (int64_t)id * 7;
    Raw r;
#pragma unroll
    for (int k = 0; k < 7; ++k) r.g[k] = g[k];
    r.f[0] = r.f[1] = r.f[2] = 0.0f;
    r.id = id;
    write_records<false>(r, alpha_threshold, s_rec + tid * 3, s_cull + tid * 2);
    if (s_id) s_id[tid] = id;
  }
  if (FEATS) {
    for (int idx = tid; idx < count * FP; idx += WIDE_THREADS) {
      const int t = idx / FP, c = idx - t * FP;
      const int32_t id = o2p[begin + t];
      s_feat[t * FS + c] = c < f ? feats[(int64_t)id * f + c] : 0.0f;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// (two waves per SIMD asked for: left alone the compiler spends 268 registers at NB = 4, one wave per SIMD, and the pass
// is then 1.75 x slower; held to 256 it needs 174 and no scratch)
template <int NB>
__global__ void __launch_bounds__(WIDE_THREADS, 2)
raster_wide_fwd_kernel(const float* __restrict__ points, const float* __restrict__ feats,
                       const int32_t* __restrict__ ranges, const int32_t* __restrict__ o2p, WideParams rp,
                       float* __restrict__ image, float* __restrict__ image_alpha) {
  constexpr int FP = 32 * NB, FS = FP + 1;
  __shared__ float4 s_rec[WIDE_BATCH * 3];
  __shared__ float4 s_cull[WIDE_BATCH * 2];
  __shared__ float s_feat[WIDE_BATCH * FS];

  const int tile_id = blockIdx.x;
  const int tile_u = tile_id % rp.tiles_wide, tile_v = tile_id / rp.tiles_wide;
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const int patch_x = tile_u * 16 + (wave & 1) * 8, patch_y = tile_v * 16 + (wave >> 1) * 8;
  const int pix_x = patch_x + (lane & 7), pix_y = patch_y + (lane >> 3);
  const float px = float(pix_x) + 0.5f, py = float(pix_y) + 0.5f;
  const float rcx = float(patch_x) + 4.0f, rcy = float(patch_y) + 4.0f;
  const bool in_bounds = pix_x < rp.width && pix_y < rp.height;
  const int col = lane & 31, half = lane >> 5;

  f32x16 acc[2][NB];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
    for (int cb = 0; cb < NB; ++cb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[rb][cb][r] = 0.0f;
    }
  }
  float W = in_bounds ? 0.0f : 1.0f;

  // blend weight of staged splat b at this lane's pixel; advances the accumulated weight
  auto blend = [&](int b) {
    const float4 r0 = s_rec[3 * b], r1 = s_rec[3 * b + 1];
    const float dx = px - r0.x, dy = py - r0.y;
    const float X = dx * r0.z + dy * r0.w, Y = dx * r1.x + dy * r1.y;
    const float p = __builtin_amdgcn_exp2f((X * X + Y * Y) * EXP2_SCALE);
    const float alpha = fminf(r1.z * p, rp.clamp_max_alpha);
    const float weight = alpha > rp.alpha_threshold ? alpha * (1.0f - W) : 0.0f;
    W += weight;
    return weight;
  };

  const int start = ranges[tile_id * 2 + 0], end = ranges[tile_id * 2 + 1];
  for (int begin = start; begin < end; begin += WIDE_BATCH) {
    const int count = (end - begin) < WIDE_BATCH ? (end - begin) : WIDE_BATCH;
    __syncthreads();   // previous batch fully consumed
    wide_stage<NB, true>(points, feats, o2p, begin, count, rp.f, rp.alpha_threshold, s_rec, s_cull, nullptr, s_feat);
    __syncthreads();

    const bool hit = lane < count && patch_hit(s_cull[2 * lane], s_cull[2 * lane + 1], rcx, rcy);
    unsigned long long m = __ballot(hit);
    while (m) {
      const int b0 = __builtin_ctzll(m);
      m &= m - 1;
      const bool pair = m != 0;
      const int b1 = pair ? __builtin_ctzll(m) : b0;
      m &= m - 1;        // (0 & -1 = 0 when there was no second hit)
      const float w0 = blend(b0);
      const float w1 = pair ? blend(b1) : 0.0f;
      if (__ballot(w0 != 0.0f || w1 != 0.0f) == 0) continue;     // the pair touches no pixel of this patch
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(w0), __float_as_uint(w1), false, false);
      const float a0 = __uint_as_float(sw[0]), a1 = __uint_as_float(sw[1]);   // pixels 0-31 / 32-63: [k = 0 | k = 1]
      const float* frow = s_feat + (half ? b1 : b0) * FS + col;
#pragma unroll
      for (int cb = 0; cb < NB; ++cb) {
        const float bv = frow[32 * cb];
        acc[0][cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc[0][cb], 0, 0, 0);
        acc[1][cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc[1][cb], 0, 0, 0);
      }
    }
  }

  if (in_bounds) image_alpha[(int64_t)pix_y * rp.width + pix_x] = W;
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int q = rb * 32 + mfma_row(r, half);
      const int x = patch_x + (q & 7), y = patch_y + (q >> 3);
      if (x < rp.width && y < rp.height) {
        float* dst = image + ((int64_t)y * rp.width + x) * rp.f;
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) {
          if (32 * cb + col < rp.f) dst[32 * cb + col] = acc[rb][cb][r];
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
template <int NB, bool GP, bool GF> struct WideBwdLds {
  static constexpr int FP = 32 * NB, FS = FP + 1;
  static constexpr int FEAT = GP ? WIDE_BATCH * FS : 1;          // staged feature rows (piece 1 only)
  static constexpr int WT = GF ? 4 * 64 * 33 : 1;                // per wave: weights [pixel][hit], rows 33 apart
  static constexpr int ACC = GF ? WIDE_BATCH * FP : 1;           // the tile's feature gradient of one batch
};

// (two workgroups per CU wherever LDS lets two fit: with both gradients at NB >= 3 it does not, and the registers are free)
template <int NB, bool GP, bool GF>
__global__ void __launch_bounds__(WIDE_THREADS, (NB >= 3 && GP && GF) ? 1 : 2)
raster_wide_bwd_kernel(const float* __restrict__ points, const float* __restrict__ feats,
                       const int32_t* __restrict__ ranges, const int32_t* __restrict__ o2p,
                       const float* __restrict__ image, const float* __restrict__ grad_image, WideParams rp,
                       float* __restrict__ grad_points, float* __restrict__ grad_feats) {
  using L = WideBwdLds<NB, GP, GF>;
  constexpr int FP = L::FP, FS = L::FS;
  __shared__ float4 s_rec[WIDE_BATCH * 3];
  __shared__ float4 s_cull[WIDE_BATCH * 2];
  __shared__ int32_t s_id[WIDE_BATCH];
  __shared__ int32_t s_hit[4][64];
  __shared__ float s_feat[L::FEAT];
  __shared__ float s_w[L::WT];
  __shared__ float s_gf[L::ACC];

  const int tile_id = blockIdx.x;
  const int tile_u = tile_id % rp.tiles_wide, tile_v = tile_id / rp.tiles_wide;
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const int patch_x = tile_u * 16 + (wave & 1) * 8, patch_y = tile_v * 16 + (wave >> 1) * 8;
  const int pix_x = patch_x + (lane & 7), pix_y = patch_y + (lane >> 3);
  const float px = float(pix_x) + 0.5f, py = float(pix_y) + 0.5f;
  const float rcx = float(patch_x) + 4.0f, rcy = float(patch_y) + 4.0f;
  const bool in_bounds = pix_x < rp.width && pix_y < rp.height;
  const int col = lane & 31, half = lane >> 5;
  const int f = rp.f;

  // piece 1's B operands: G[pixel 32 pb + col][channel 2 step + half], zero outside the image and the channels
  float Gp[2][GP ? FP / 2 : 1];
  float Q = 0.0f;        // G[p].C[p] minus what the splats up to here have blended: the remaining "colour" of g
  if (GP) {
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
      const int q = pb * 32 + col;
      const int x = patch_x + (q & 7), y = patch_y + (q >> 3);
      const bool ok = x < rp.width && y < rp.height;
      const float* src = grad_image + ((int64_t)(ok ? y : 0) * rp.width + (ok ? x : 0)) * f;
#pragma unroll
      for (int step = 0; step < FP / 2; ++step) {
        const int c = 2 * step + half;
        Gp[pb][step] = (ok && c < f) ? src[c] : 0.0f;
      }
    }
    if (in_bounds) {
      const int64_t p = ((int64_t)pix_y * rp.width + pix_x) * f;
      for (int c = 0; c < f; ++c) Q += image[p + c] * grad_image[p + c];
    }
  }
  if (GF) {
    for (int idx = threadIdx.x; idx < WIDE_BATCH * FP; idx += WIDE_THREADS) s_gf[idx] = 0.0f;
  }
  float W = in_bounds ? 0.0f : 1.0f;
  float* const wrow = s_w + (GF ? wave * 64 * 33 : 0);

  // which word of grad_points7 this lane commits after wave_reduce16
  const int slot = butterfly_slot(lane);
  const bool commits = (lane & 15) >= 12 && slot < 7;

  const int start = ranges[tile_id * 2 + 0], end = ranges[tile_id * 2 + 1];
  for (int begin = start; begin < end; begin += WIDE_BATCH) {
    const int count = (end - begin) < WIDE_BATCH ? (end - begin) : WIDE_BATCH;
    // tile-wide early out once every pixel is saturated (backward.py:116); also: previous batch consumed and committed
    if (__syncthreads_and(W >= rp.saturate_threshold)) break;
    wide_stage<NB, GP>(points, feats, o2p, begin, count, f, rp.alpha_threshold, s_rec, s_cull, s_id, s_feat);
    __syncthreads();

    if (__ballot(W < rp.saturate_threshold) != 0) {       // wave-wide early out (backward.py:142)
      const bool hit = lane < count && patch_hit(s_cull[2 * lane], s_cull[2 * lane + 1], rcx, rcy);
      unsigned long long m = __ballot(hit);
      const int n = __popcll(m);
      if (hit) s_hit[wave][lane_rank_popc(m)] = lane;
      wave_lds_fence();

      for (int g0 = 0; g0 < n; g0 += 32) {
        const int cnt = (n - g0) < 32 ? (n - g0) : 32;

        // ---- 1. g of the 32 hits at this lane's pixel: ga[r] = hit mfma_row(r, 0), gb[r] = hit mfma_row(r, 1)
        float ga[GP ? 16 : 1], gb[GP ? 16 : 1];
        if (GP) {
          const float* frow = s_feat + s_hit[wave][g0 + (col < cnt ? col : 0)] * FS + half;
          f32x16 d0, d1;
#pragma unroll
          for (int r = 0; r < 16; ++r) { d0[r] = 0.0f; d1[r] = 0.0f; }
#pragma unroll
          for (int step = 0; step < FP / 2; ++step) {
            const float a = frow[2 * step];
            d0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Gp[0][step], d0, 0, 0, 0);
            d1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Gp[1][step], d1, 0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(d0[r]), __float_as_uint(d1[r]), false, false);
            ga[r] = __uint_as_float(sw[0]);
            gb[r] = __uint_as_float(sw[1]);
          }
        }

        // ---- 2. the scalar chain, hit by hit in list order
#pragma unroll
        for (int j = 0; j < 32; ++j) {
          if (j < cnt) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            const float4 r0 = s_rec[3 * b], r1 = s_rec[3 * b + 1];
            const float dx = px - r0.x, dy = py - r0.y;
            const float X = dx * r0.z + dy * r0.w, Y = dx * r1.x + dy * r1.y;
            const float p = __builtin_amdgcn_exp2f((X * X + Y * Y) * EXP2_SCALE);
            const float alpha_raw = r1.z * p;
            const bool active = alpha_raw > rp.alpha_threshold && W < rp.saturate_threshold;
            const float alpha = fminf(alpha_raw, rp.clamp_max_alpha);
            const float Ti = 1.0f - W;
            const float weight = active ? alpha * Ti : 0.0f;
            W += weight;
            if (GF) wrow[lane * 33 + j] = weight;
            if (GP) {
              const float g = ((j >> 2) & 1) ? gb[(j & 3) + 4 * (j >> 3)] : ga[(j & 3) + 4 * (j >> 3)];
              Q -= weight * g;
              const float alpha_grad = active ? g * Ti - Q * __builtin_amdgcn_rcpf(1.0f - alpha) : 0.0f;
              if (__ballot(active) != 0) {
                const float4 r2 = s_rec[3 * b + 2];
                const float aag = r1.z * alpha_grad;      // straight-through clamp (backward.py:158-163)
                const float pX = p * X, pY = p * Y;
                const float u = pX * r2.z, w = pY * r2.w;
                float v[16];
                v[0] = aag * (pX * r0.z + pY * r1.x);     // dp/dmean
                v[1] = aag * (pX * r0.w + pY * r1.y);
                v[2] = aag * -(u * dx + w * dy);          // dp/daxis
                v[3] = aag * (w * dx - u * dy);
                v[4] = aag * (u * X);                     // dp/dsigma
                v[5] = aag * (w * Y);
                v[6] = p * alpha_grad;
#pragma unroll
                for (int k = 7; k < 16; ++k) v[k] = 0.0f;
                const float total = wave_reduce16(v, lane & 1, lane & 2);
                if (commits) atomic_add_noret(grad_points + (int64_t)s_id[b] * 7 + slot, total);
              }
            }
          }
        }

        // ---- 3. grad_feats of the 32 hits from this wave's 64 pixels
        if (GF) {
          wave_lds_fence();
#pragma unroll
          for (int cb = 0; cb < NB; ++cb) {
            const int c = 32 * cb + col;
            f32x16 d;
#pragma unroll
            for (int r = 0; r < 16; ++r) d[r] = 0.0f;
            // the loads of CH steps are issued before the first product waits for one: 32 / CH trips to L1 / L2 per block
            // (CH = 16 where the registers allow it next to piece 1's operands)
            constexpr int CH = (GP && NB >= 2) ? 8 : 16;
            constexpr int UNROLL_CHUNKS = CH == 8 ? 1 : 2;       // (rolled where unrolling would hoist every load: spills)
#pragma unroll UNROLL_CHUNKS
            for (int h0 = 0; h0 < 32; h0 += CH) {
              float bv[CH];
#pragma unroll
              for (int k = 0; k < CH; ++k) {
                const int q = 2 * (h0 + k) + half;
                const int x = patch_x + (q & 7), y = patch_y + (q >> 3);
                const bool ok = x < rp.width && y < rp.height && c < f;
                bv[k] = ok ? grad_image[((int64_t)y * rp.width + x) * f + c] : 0.0f;
              }
#pragma unroll
              for (int k = 0; k < CH; ++k)
                d = __builtin_amdgcn_mfma_f32_32x32x2f32(wrow[(2 * (h0 + k) + half) * 33 + col], bv[k], d, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int row = mfma_row(r, half);
              if (row < cnt && d[r] != 0.0f) {
                __hip_atomic_fetch_add(&s_gf[s_hit[wave][g0 + row] * FP + c], d[r], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
              }
            }
          }
          wave_lds_fence();
        }
      }
    }

    if (GF) {
      __syncthreads();     // every wave has added its tiles
      for (int idx = threadIdx.x; idx < count * FP; idx += WIDE_THREADS) {
        const float v = s_gf[idx];
        if (v != 0.0f) {
          const int t = idx / FP, c = idx - t * FP;
          if (c < f) atomic_add_noret(grad_feats + (int64_t)s_id[t] * f + c, v);
          s_gf[idx] = 0.0f;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
static int wide_check(const char* who, const ms_raster_config* cfg, bool pointers, int image_w, int image_h, int f,
                      bool outputs) {
  if (!cfg || !pointers) { set_error("%s: null pointer", who); return MS_ERR_BAD_ARG; }
  if (image_w <= 0 || image_h <= 0) { set_error("%s: bad image size %dx%d", who, image_w, image_h); return MS_ERR_BAD_ARG; }
  if (f < 1 || f > MS_RASTER_WIDE_MAX_F) {
    set_error("%s: feature size %d outside 1..%d", who, f, MS_RASTER_WIDE_MAX_F);
    return MS_ERR_BAD_ARG;
  }
  if (!outputs) { set_error("%s: grad_points7 and grad_features are both null", who); return MS_ERR_BAD_ARG; }
  if (cfg->tile_size != 16) { set_error("%s: tile_size must be 16 (got %d)", who, cfg->tile_size); return MS_ERR_UNSUPPORTED; }
  if (cfg->antialias) { set_error("%s: antialias is not supported by the wide rasteriser", who); return MS_ERR_UNSUPPORTED; }
  if (!cfg->use_alpha_blending) { set_error("%s: the wide rasteriser requires use_alpha_blending", who); return MS_ERR_UNSUPPORTED; }
  return 0;
}

static WideParams make_wide_params(const ms_raster_config* cfg, int image_w, int image_h, int f) {
  WideParams rp;
  rp.width = image_w; rp.height = image_h; rp.tiles_wide = (image_w + 15) / 16; rp.f = f;
  rp.clamp_max_alpha = (float)cfg->clamp_max_alpha;
  rp.alpha_threshold = (float)cfg->alpha_threshold;
  rp.saturate_threshold = (float)cfg->saturate_threshold;
  return rp;
}

}  // namespace ms

using namespace ms;

extern "C" int ms_raster_wide_fwd(const float* points7, const float* features, const int32_t* tile_ranges,
                                  const int32_t* overlap_to_point, int image_w, int image_h, int f,
                                  const ms_raster_config* cfg, float* out_image, float* out_alpha, void* stream) {
  if (const int rc = wide_check(__func__, cfg, points7 && features && tile_ranges && overlap_to_point && out_image && out_alpha,
                                image_w, image_h, f, true)) return rc;
  const WideParams rp = make_wide_params(cfg, image_w, image_h, f);
  const unsigned tiles = (unsigned)rp.tiles_wide * (unsigned)((image_h + 15) / 16);
  with_constant<1, 2, 3, 4>((f + 31) / 32, [&](auto nb) {
    raster_wide_fwd_kernel<decltype(nb)::value><<<dim3(tiles), dim3(WIDE_THREADS), 0, (hipStream_t)stream>>>(
        points7, features, tile_ranges, overlap_to_point, rp, out_image, out_alpha);
  });
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_raster_wide_bwd(const float* points7, const float* features, const int32_t* tile_ranges,
                                  const int32_t* overlap_to_point, const float* image, const float* grad_image,
                                  int image_w, int image_h, int f, const ms_raster_config* cfg, float* grad_points7,
                                  float* grad_features, void* stream) {
  if (const int rc = wide_check(__func__, cfg, points7 && features && tile_ranges && overlap_to_point && image && grad_image,
                                image_w, image_h, f, grad_points7 || grad_features)) return rc;
  const WideParams rp = make_wide_params(cfg, image_w, image_h, f);
  const unsigned tiles = (unsigned)rp.tiles_wide * (unsigned)((image_h + 15) / 16);
  with_constant<1, 2, 3, 4>((f + 31) / 32, [&](auto nb) {
    auto launch = [&](auto gp, auto gf) {
      raster_wide_bwd_kernel<decltype(nb)::value, decltype(gp)::value, decltype(gf)::value>
          <<<dim3(tiles), dim3(WIDE_THREADS), 0, (hipStream_t)stream>>>(
              points7, features, tile_ranges, overlap_to_point, image, grad_image, rp, grad_points7, grad_features);
    };
    if (grad_points7 && grad_features) launch(std::true_type{}, std::true_type{});
    else if (grad_points7) launch(std::true_type{}, std::false_type{});
    else launch(std::false_type{}, std::true_type{});
  });
  MS_CHECK_LAUNCH();
  return 0;
}
