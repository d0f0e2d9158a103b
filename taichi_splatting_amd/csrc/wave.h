// wave.h — the wave64 and block primitives every kernel file shares (included by common.h).  A new kernel calls these;
// it does not write its own butterfly, scan ladder or ballot rank.  All 64 lanes are active at every call unless noted.
// Deliberately NOT here (single use, tuned with their kernel; leave them where they are): wave_reduce16 / wave_reduce4 /
// butterfly_slot, min_f32* and wave_lds_fence (raster_common.h); the inline-assembly scans wave_scan_mul2 / wave_scan_add2
// (raster_bwd_shared.h); the (score, index) pair minimum over 32 lanes (kmeans.hip); the ballot loop of the union-find
// (mesh.hip); wave_broadcast / readlane_f (mapper.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ms {

constexpr int WAVE = 64;

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

// DPP move: returns src shuffled by the DPP control, lanes without a source keep `old`.
template <int CTRL, int ROW_MASK = 0xf, int BANK_MASK = 0xf, bool BOUND_CTRL = false>
__device__ __forceinline__ float dpp_f32(float old, float src) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), CTRL,
                                                    ROW_MASK, BANK_MASK, BOUND_CTRL));
}

// keep + (send of the lane the DPP control names); a lane without a source adds 0 (bound_ctrl).
template <int CTRL>
__device__ __forceinline__ float add_dpp(float keep, float send) {
  return keep + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(send), CTRL, 0xf, 0xf, true));
}

// v of the lane the DPP control names (two 32-bit moves); a lane without a source keeps its own v.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false),
                          __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false));
}

// Sum over the 16 lanes of a DPP row, the same bits in every lane of the row.
__device__ __forceinline__ double row_sum16(double v) {
  v += dpp_f64<0xb1>(v);                            // quad_perm:[1,0,3,2]   lane ^ 1
  v += dpp_f64<0x4e>(v);                            // quad_perm:[2,3,0,1]   lane ^ 2
  v += dpp_f64<0x141>(v);                           // row_half_mirror       the other quad of the half
  v += dpp_f64<0x140>(v);                           // row_mirror            the other half of the row
  return v;
}

// Xor butterfly over aligned groups of LANES lanes (a power of two <= 64): every lane gets op over its group, folded as
// v = op(v, partner's v) from distance LANES / 2 down to 1.  op: any (T, T) -> T; T: what __shfl_xor moves (unsigned
// goes through int).
template <int LANES, typename T, typename Op>
__device__ __forceinline__ T group_all(T v, Op op) {
#pragma unroll
  for (int off = LANES / 2; off >= 1; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
  return v;
}
// The 64-lane case: op over the wave, in every lane.
template <typename T, typename Op>
__device__ __forceinline__ T wave_all(T v, Op op) { return group_all<64>(v, op); }

// Sum over the 64 lanes of a wave; the total is valid in lane 63 (other lanes hold partials).
// row_shr:1,2,4,8 build row (16-lane) totals in lane 15 of each row, row_bcast:15 / row_bcast:31
// carry them across rows — 6 VALU+DPP instructions per value, no LDS traffic.  This replaces the
// reference's 32-lane shfl_down tree + shared-memory atomics (taichi_lib/concurrent.py:11-23,69-86).
__device__ __forceinline__ float wave_sum_to_lane63(float v) {
  v += dpp_f32<0x111>(0.f, v);                    // row_shr:1
  v += dpp_f32<0x112>(0.f, v);                    // row_shr:2
  v += dpp_f32<0x114>(0.f, v);                    // row_shr:4
  v += dpp_f32<0x118>(0.f, v);                    // row_shr:8
  v += dpp_f32<0x142, 0xa>(0.f, v);               // row_bcast:15 -> rows 1 and 3
  v += dpp_f32<0x143, 0xc>(0.f, v);               // row_bcast:31 -> rows 2 and 3
  return v;
}

// f64 path (gradcheck-style tests only): plain xor butterfly through ds_bpermute, valid in every lane.
__device__ __forceinline__ double wave_sum_to_lane63(double v) {
  return wave_all(v, [](double a, double b) { return a + b; });
}

// Inclusive prefix sum over the wave (__shfl_up ladder): lane l gets v of lanes 0 .. l, lane 63 the wave total.
template <typename T>
__device__ __forceinline__ T wave_inclusive_sum(T v) {
  const int lane = lane_id();
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const T t = __shfl_up(v, off, 64); if (lane >= off) v += t; }
  return v;
}

// Exclusive prefix sum of one value per thread over a block of WAVES waves; *total = the block sum, in every thread.
// ONE __syncthreads() inside, between writing and reading red[0 .. WAVES), and NONE that protects red between two calls:
// a caller that calls again, or reuses red, owes a barrier in between.  Every thread of the block must call.
template <int WAVES, typename T>
__device__ __forceinline__ T block_exclusive_sum(T v, T* red, T* total) {
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const T inc = wave_inclusive_sum(v);
  if (lane == 63) red[wave] = inc;
  __syncthreads();
  T before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) { const T c = red[w]; if (w < wave) before += c; all += c; }
  *total = all;
  return before + inc - v;
}

// Set bits of mask (a __ballot) below the calling lane; any lane may call.  Two spellings that compile differently
// (v_mbcnt pair against 64-bit shift, and, popcount): a kernel keeps the one it was tuned with.
__device__ __forceinline__ int lane_rank_mbcnt(unsigned long long mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
__device__ __forceinline__ int lane_rank_popc(unsigned long long mask) {
  return __popcll(mask & ((1ull << lane_id()) - 1ull));
}

__device__ __forceinline__ float atomic_add(float* p, float v) { return atomicAdd(p, v); }
__device__ __forceinline__ double atomic_add(double* p, double v) { return atomicAdd(p, v); }

// fire-and-forget float atomic add (no return value => global_atomic_add_f32 without glc)
__device__ __forceinline__ void atomic_add_noret(float* p, float v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void atomic_add_noret(double* p, double v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Sum NV per-thread values over a 256-thread block and add the block totals to dst[0..NV) with ONE atomic per
// value per block (wave DPP reduce -> LDS -> first NV threads).  For whole-launch sums (camera gradients):
// combined with a grid-stride loop over a bounded number of blocks this keeps the same-address atomic count
// in the thousands instead of one per wave.  Every thread must call; one __syncthreads() inside, none around lds.
template <typename T, int NV>
__device__ __forceinline__ void block_sum_commit(const T (&v)[NV], T* __restrict__ dst, T* lds /* >= 4 * NV */) {
  const int lane = lane_id(), wave = threadIdx.x >> 6, waves = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const T s = wave_sum_to_lane63(v[k]);
    if (lane == 63) lds[wave * NV + k] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < NV) {
    T t = T(0);
    for (int w = 0; w < waves; ++w) t += lds[w * NV + threadIdx.x];
    if (t != T(0)) atomic_add_noret(dst + threadIdx.x, t);
  }
}

// The integer sibling: wave_total is wave-uniform already (a sum of ballot popcounts); the four waves of a 256-thread
// block add up in LDS of its own and thread 0 commits ONE 64-bit atomic.  Every thread must call; a second call in the
// same kernel needs a __syncthreads() before it.
__device__ __forceinline__ void block_count_commit(uint32_t wave_total, int64_t* dst) {
  __shared__ uint32_t totals[4];
  if (lane_id() == 0) totals[threadIdx.x >> 6] = wave_total;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t t = totals[0] + totals[1] + totals[2] + totals[3];
    if (t != 0) atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)t);
  }
}

}  // namespace ms
