// camera_coverage.hip — which cameras of a set see each gaussian, in ONE launch (no reference counterpart: the
// reference, like this package until now, looks at a scene through one camera at a time).
//
// One lane per gaussian; the lane loops over all C cameras and takes, for each, bit for bit the in_view decision
// ms_project_fwd takes for that camera (project_forward of splat_math.h, same flags, no FMA contraction: the culling
// comparisons are shared with projection.hip and the oracle).  Per gaussian it writes
//   count      number of cameras that have it in view
//   max_rate   max over those cameras of max(fx, fy) / z, one division in T (0 where count == 0)
//   min_depth  min over those cameras of z = pc[2]                        (+inf where count == 0)
//   mask       optional, (ceil(C / 32), n) words, WORD-major: consecutive lanes store consecutive words; bit c % 32 of
//              mask[c / 32][i] <=> camera c sees gaussian i; the unused high bits of the last word are zero
// Instantiations: camera_coverage_kernel<T> for T in {float, double} = 2 (tests/test_camera_coverage_budgets.py holds
// the count, 0 bytes of scratch, <= 64 VGPRs in float32 and <= 128 in float64).
//
// Shape: the gaussian (11 values) is read once and stays in registers.  The camera rows (MS_COVERAGE_CAMERA_VALUES = 20
// values each, a few kilobytes for the whole set) are indexed by the loop counter alone, so every lane of a wave reads
// the same addresses: the compiler fetches them through the scalar cache into SGPRs, no lane loads them.  What does not
// depend on the camera (quaternion normalisation and rotation matrix, exp of the scales, the sigmoid and the
// alpha-threshold radius) is loop-invariant and hoisted by the compiler.
// Early-out: z > near && z < far is part of the decision and needs only pc[2]; a lane that fails it skips the
// covariance and eigen work for that camera, and a wave whose lanes all fail it branches over that code.  The z it
// tests is the same expression project_forward evaluates, so no result changes.
// No atomics anywhere: the outputs are bitwise reproducible.  HBM traffic: 44 B in, 12 + 4 ceil(C / 32) B out per
// gaussian in float32; the kernel is compute bound from a few cameras on.
#pragma clang fp contract(off)
#include "common.h"

namespace ms {

constexpr int COVERAGE_CAMERA = MS_COVERAGE_CAMERA_VALUES;
static_assert(COVERAGE_CAMERA == 20, "T_camera_world rows 0..2 | fx fy cx cy | near far | width height");

template <typename T>
__global__ void __launch_bounds__(256)
camera_coverage_kernel(const T* __restrict__ position, const T* __restrict__ log_scaling,
                       const T* __restrict__ rotation, const T* __restrict__ alpha_logit,
                       const T* __restrict__ cameras, int num_cameras, T blur_cov, T clamp_margin, T alpha_threshold,
                       int64_t n, int32_t* __restrict__ out_count, T* __restrict__ out_max_rate,
                       T* __restrict__ out_min_depth, uint32_t* __restrict__ out_mask) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;

  const T p[3] = {position[i * 3 + 0], position[i * 3 + 1], position[i * 3 + 2]};
  const T ls[3] = {log_scaling[i * 3 + 0], log_scaling[i * 3 + 1], log_scaling[i * 3 + 2]};
  const T q[4] = {rotation[i * 4 + 0], rotation[i * 4 + 1], rotation[i * 4 + 2], rotation[i * 4 + 3]};
  const T al = alpha_logit[i];

  int32_t count = 0;
  T max_rate = T(0);
  T min_depth = T(__builtin_huge_val());

#pragma unroll 1
  for (int first = 0; first < num_cameras; first += 32) {
    const int in_word = num_cameras - first < 32 ? num_cameras - first : 32;
    uint32_t word = 0;
#pragma unroll 1
    for (int b = 0; b < in_word; ++b) {
      const T* __restrict__ row = cameras + (int64_t)(first + b) * COVERAGE_CAMERA;   // wave-uniform
      Camera<T> cam;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) cam.t[r][c] = row[r * 4 + c];
      ProjParams<T> pp;
      pp.near_plane = row[16]; pp.far_plane = row[17];

      // pc[2] exactly as project_forward forms it
      const T z = cam.t[2][0] * p[0] + cam.t[2][1] * p[1] + cam.t[2][2] * p[2] + cam.t[2][3];
      if (!((z > pp.near_plane) && (z < pp.far_plane))) continue;

      cam.fx = row[12]; cam.fy = row[13]; cam.cx = row[14]; cam.cy = row[15];
      pp.width = row[18]; pp.height = row[19];
      pp.blur_cov = blur_cov; pp.clamp_margin = clamp_margin; pp.alpha_threshold = alpha_threshold;

      ProjState<T> st;
      if (project_forward(p, ls, q, al, cam, pp, st)) {
        word |= 1u << b;
        ++count;
        max_rate = t_max(max_rate, t_max(cam.fx, cam.fy) / st.pc[2]);
        min_depth = t_min(min_depth, st.pc[2]);
      }
    }
    if (out_mask) out_mask[(int64_t)(first >> 5) * n + i] = word;     // words * n can pass 2^31
  }

  out_count[i] = count;
  out_max_rate[i] = max_rate;
  out_min_depth[i] = min_depth;
}

template <typename T>
static int launch_camera_coverage(const void* position, const void* log_scaling, const void* rotation,
                                  const void* alpha_logit, const void* cameras, int num_cameras, double blur_cov,
                                  double clamp_margin, double alpha_threshold, int64_t n, int32_t* out_count,
                                  void* out_max_rate, void* out_min_depth, uint32_t* out_mask, hipStream_t stream) {
  camera_coverage_kernel<T><<<dim3((unsigned)div_up(n, 256)), dim3(256), 0, stream>>>(
      (const T*)position, (const T*)log_scaling, (const T*)rotation, (const T*)alpha_logit, (const T*)cameras,
      num_cameras, (T)blur_cov, (T)clamp_margin, (T)alpha_threshold, n, out_count, (T*)out_max_rate,
      (T*)out_min_depth, out_mask);
  MS_CHECK_LAUNCH();
  return 0;
}

}  // namespace ms

using namespace ms;

extern "C" int ms_camera_coverage(const void* position, const void* log_scaling, const void* rotation,
                                  const void* alpha_logit, const void* cameras, int num_cameras, double blur_cov,
                                  double clamp_margin, double alpha_threshold, int64_t n, int32_t* out_count,
                                  void* out_max_rate, void* out_min_depth, uint32_t* out_mask, int dtype, void* stream) {
  MS_CHECK_ARG(n >= 0, "n >= 0 expected");
  MS_CHECK_ARG(n <= INT32_MAX, "n < 2^31 expected");
  MS_CHECK_ARG(num_cameras >= 1 && num_cameras <= MS_COVERAGE_MAX_CAMERAS, "1 <= num_cameras <= 65535 expected");
  MS_CHECK_ARG(dtype == MS_F32 || dtype == MS_F64, "dtype must be MS_F32 or MS_F64");
  MS_CHECK_ARG(aligned(dtype == MS_F64 ? 8 : 4, {position, log_scaling, rotation, alpha_logit, cameras, out_max_rate, out_min_depth}),
               "every pointer must be aligned to its element type");
  MS_CHECK_ARG(aligned(4, {out_count, out_mask}), "out_count and out_mask must be aligned to 4 bytes");
  if (n == 0) return 0;
  MS_CHECK_ARG(position && log_scaling && rotation && alpha_logit, "null gaussian input");
  MS_CHECK_ARG(cameras != nullptr, "null cameras");
  MS_CHECK_ARG(out_count && out_max_rate && out_min_depth, "null output");      // out_mask may be NULL (no masks)
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MS_F32)
    return launch_camera_coverage<float>(position, log_scaling, rotation, alpha_logit, cameras, num_cameras, blur_cov,
                                         clamp_margin, alpha_threshold, n, out_count, out_max_rate, out_min_depth,
                                         out_mask, s);
  return launch_camera_coverage<double>(position, log_scaling, rotation, alpha_logit, cameras, num_cameras, blur_cov,
                                        clamp_margin, alpha_threshold, n, out_count, out_max_rate, out_min_depth,
                                        out_mask, s);
}
