// scene_transform.hip — a similarity transform m = [[s R, t], [0, 1]] applied to a whole 3-D scene in ONE launch:
//   position' = s R p + t      log_scaling' = log_scaling + ln s      rotation' = q_R (x) q  (xyzw, not normalised)
//   feature'  : every (gaussian, channel) vector of (D + 1)^2 SH coefficients, band by band, c'_l = M_l(R) c_l
// (band 0 is invariant; alpha_logit and plain colours do not change and are not arguments).  No reference counterpart:
// the reference's transform_rigid (data_types.py:91-102) moves position and rotation and leaves the SH bands alone.
//
// Instantiations: scene_transform_kernel<T, DEG> for T in {float, double} x DEG in {0, 1, 2, 3} = 8, DEG 0 being the
// launch without a feature (tests/test_scene_transform_budgets.py holds the count and 0 bytes of scratch).
//
// Shape: a workgroup of 256 lanes takes MS_SCENE_XFORM_ROWS = 256 consecutive rows.
//   geometry  one lane per row, each field on its own (12, 12 and 16 bytes per row: the wave's loads of a field cover
//             one contiguous range).  Evaluated in double from the stored values and rounded once: the float32 result
//             is the correctly rounded one, whatever ln s or t cancel against.
//   feature   the block's rows are f * 256 vectors of K = (D + 1)^2 coefficients, a contiguous byte range.  It moves in
//             chunks of 256 vectors through LDS: 16-byte coalesced pieces global -> LDS, one vector per lane rotated in
//             place in LDS (at most 9 + 25 + 49 = 83 FMAs), 16-byte pieces LDS -> global.  A chunk starts a multiple of
//             256 K sizeof(T) bytes from the base, so its alignment is the base's: with both bases 16-byte aligned the
//             chunk moves as 16-byte pieces plus a tail of 4-byte pieces (the last chunk of a degree-2 float32 tensor
//             is 36 bytes per vector), otherwise (a sliced tensor) as 4-byte pieces throughout.  A chunk is read
//             completely before any of it is written, and chunks are disjoint: out == in works in place.
// The transform is uniform over the launch and travels in the kernel arguments (scalar registers / scalar loads), the
// matrices already rounded to T on the host: no lane loads it from a buffer.
// LDS: the degree-3 float32 vector is 64 bytes, so the per-lane 16-byte LDS accesses of the rotate phase are 4-way
// bank conflicted; with the two copy phases that is about 1000 LDS cycles per 16 KiB chunk, a quarter of the time the
// CU's share of HBM needs for the same chunk, so the rows are not padded (padding would break the straight copy).
// HBM traffic: every given field read once and written once.
#include "common.h"

namespace ms {

constexpr int XFORM_ROWS = MS_SCENE_XFORM_ROWS;   // rows per workgroup = lanes per workgroup = vectors per LDS chunk
constexpr int XFORM_UNROLL = 4;                   // pieces in flight per lane of the chunk copies (rows.h)
static_assert(XFORM_ROWS == ROW_BLOCK, "one lane per row of the block");

template <typename T>
struct SceneXformArgs {
  const T* position; T* out_position;
  const T* log_scaling; T* out_log_scaling;
  const T* rotation; T* out_rotation;
  const T* feature; T* out_feature;
  int64_t n;
  int32_t f, vec16;
  double srt[12], ln_s, q[4];      // MS_SCENE_XFORM_* of the header, in double for the geometry
  T m[83];                         // M_1 (3x3) | M_2 (5x5) | M_3 (7x7), row-major
};

__device__ __forceinline__ float xf_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double xf_fma(double a, double b, double c) { return fma(a, b, c); }

// c[0 .. W) <- M c[0 .. W), M (W x W) row-major
template <typename T, int W>
__device__ __forceinline__ void rotate_band(const T* __restrict__ m, T* c) {
  T o[W];
#pragma unroll
  for (int i = 0; i < W; ++i) {
    T acc = m[i * W] * c[0];
#pragma unroll
    for (int j = 1; j < W; ++j) acc = xf_fma(m[i * W + j], c[j], acc);
    o[i] = acc;
  }
#pragma unroll
  for (int i = 0; i < W; ++i) c[i] = o[i];
}

// One lane's vector between LDS and registers: whole 16-byte pieces where the vector is a multiple of 16 bytes (band 0
// rides along unchanged, which keeps the accesses aligned), else element by element above band 0.
template <typename T, int K>
__device__ __forceinline__ void lds_vector(T* v, T* c, bool store) {
  constexpr int BYTES = K * (int)sizeof(T);
  if constexpr (BYTES % 16 == 0) {
    piece16 raw[BYTES / 16];
    if (store) {
      __builtin_memcpy(raw, v, BYTES);
#pragma unroll
      for (int i = 0; i < BYTES / 16; ++i) reinterpret_cast<piece16*>(c)[i] = raw[i];
    } else {
#pragma unroll
      for (int i = 0; i < BYTES / 16; ++i) raw[i] = reinterpret_cast<const piece16*>(c)[i];
      __builtin_memcpy(v, raw, BYTES);
    }
  } else {
#pragma unroll
    for (int k = 1; k < K; ++k) {
      if (store) c[k] = v[k];
      else v[k] = c[k];
    }
  }
}

template <typename T, int DEG>
__global__ void __launch_bounds__(XFORM_ROWS)
scene_transform_kernel(const SceneXformArgs<T> a) {
  const int64_t first = (int64_t)blockIdx.x * XFORM_ROWS;
  const int64_t left = a.n - first;
  const int rows = left < XFORM_ROWS ? (int)left : XFORM_ROWS;
  const int64_t row = first + threadIdx.x;

  if ((int)threadIdx.x < rows) {
    if (a.position) {
      const double x = (double)a.position[row * 3], y = (double)a.position[row * 3 + 1], z = (double)a.position[row * 3 + 2];
#pragma unroll
      for (int k = 0; k < 3; ++k)
        a.out_position[row * 3 + k] = (T)(fma(a.srt[k * 4], x, fma(a.srt[k * 4 + 1], y, fma(a.srt[k * 4 + 2], z, a.srt[k * 4 + 3]))));
    }
    if (a.log_scaling) {
      const double l0 = (double)a.log_scaling[row * 3], l1 = (double)a.log_scaling[row * 3 + 1], l2 = (double)a.log_scaling[row * 3 + 2];
      a.out_log_scaling[row * 3] = (T)(l0 + a.ln_s);
      a.out_log_scaling[row * 3 + 1] = (T)(l1 + a.ln_s);
      a.out_log_scaling[row * 3 + 2] = (T)(l2 + a.ln_s);
    }
    if (a.rotation) {
      // Hamilton product q_R (x) q, xyzw: R(q_R (x) q) = R(q_R) R(q)
      const double x = (double)a.rotation[row * 4], y = (double)a.rotation[row * 4 + 1], z = (double)a.rotation[row * 4 + 2],
                   w = (double)a.rotation[row * 4 + 3];
      const double ax = a.q[0], ay = a.q[1], az = a.q[2], aw = a.q[3];
      a.out_rotation[row * 4] = (T)(aw * x + ax * w + ay * z - az * y);
      a.out_rotation[row * 4 + 1] = (T)(aw * y - ax * z + ay * w + az * x);
      a.out_rotation[row * 4 + 2] = (T)(aw * z + ax * y - ay * x + az * w);
      a.out_rotation[row * 4 + 3] = (T)(aw * w - ax * x - ay * y - az * z);
    }
  }

  if constexpr (DEG >= 1) {
    constexpr int K = (DEG + 1) * (DEG + 1);
    __shared__ __attribute__((aligned(16))) T lds[XFORM_ROWS * K];
    const int64_t v_begin = first * a.f, v_end = (first + rows) * a.f;
    const bool vec16 = a.vec16 != 0;
#pragma unroll 1
    for (int64_t v0 = v_begin; v0 < v_end; v0 += XFORM_ROWS) {
      const int count = v_end - v0 < XFORM_ROWS ? (int)(v_end - v0) : XFORM_ROWS;
      const uint32_t bytes = (uint32_t)count * (uint32_t)(K * sizeof(T));
      copy_range<XFORM_UNROLL>(lds, a.feature + v0 * K, bytes, vec16);
      __syncthreads();
      if ((int)threadIdx.x < count) {
        T* c = lds + threadIdx.x * K;      // this lane's vector: nobody else touches it between the two barriers
        T v[K];
        lds_vector<T, K>(v, c, false);
        rotate_band<T, 3>(a.m, v + 1);
        if constexpr (DEG >= 2) rotate_band<T, 5>(a.m + 9, v + 4);
        if constexpr (DEG >= 3) rotate_band<T, 7>(a.m + 34, v + 9);
        lds_vector<T, K>(v, c, true);
      }
      __syncthreads();
      copy_range<XFORM_UNROLL>(a.out_feature + v0 * K, lds, bytes, vec16);
      __syncthreads();                     // the next chunk's loads overwrite the LDS image
    }
  }
}

template <typename T, int DEG>
static int launch_scene_transform(const SceneXformArgs<T>& a, hipStream_t stream) {
  scene_transform_kernel<T, DEG><<<dim3((unsigned)div_up(a.n, XFORM_ROWS)), dim3(XFORM_ROWS), 0, stream>>>(a);
  MS_CHECK_LAUNCH();
  return 0;
}

template <typename T>
static int scene_transform_typed(const void* position, void* out_position, const void* log_scaling, void* out_log_scaling,
                                 const void* rotation, void* out_rotation, const void* feature, void* out_feature,
                                 int64_t n, int f, int sh_degree, const double* t, hipStream_t stream) {
  SceneXformArgs<T> a{};
  a.position = (const T*)position; a.out_position = (T*)out_position;
  a.log_scaling = (const T*)log_scaling; a.out_log_scaling = (T*)out_log_scaling;
  a.rotation = (const T*)rotation; a.out_rotation = (T*)out_rotation;
  a.feature = (const T*)feature; a.out_feature = (T*)out_feature;
  a.n = n; a.f = f;
  a.vec16 = aligned(16, {feature, out_feature});
  for (int k = 0; k < 12; ++k) a.srt[k] = t[MS_SCENE_XFORM_SRT + k];
  a.ln_s = t[MS_SCENE_XFORM_LN_S];
  for (int k = 0; k < 4; ++k) a.q[k] = t[MS_SCENE_XFORM_QUAT + k];
  for (int k = 0; k < 83; ++k) a.m[k] = (T)t[MS_SCENE_XFORM_M1 + k];      // rounded once
  switch (feature ? sh_degree : 0) {
    case 0: return launch_scene_transform<T, 0>(a, stream);
    case 1: return launch_scene_transform<T, 1>(a, stream);
    case 2: return launch_scene_transform<T, 2>(a, stream);
    default: return launch_scene_transform<T, 3>(a, stream);
  }
}

}  // namespace ms

using namespace ms;

extern "C" int ms_scene_transform(const void* position, void* out_position, const void* log_scaling, void* out_log_scaling,
                                  const void* rotation, void* out_rotation, const void* feature, void* out_feature,
                                  int64_t n, int f, int sh_degree, int dtype, const double* transform_host, void* stream) {
  MS_CHECK_ARG(n >= 0, "n >= 0 expected");
  MS_CHECK_ARG(n <= INT32_MAX, "n < 2^31 expected");
  MS_CHECK_ARG(dtype == MS_F32 || dtype == MS_F64, "dtype must be MS_F32 or MS_F64");
  MS_CHECK_ARG((position == nullptr) == (out_position == nullptr), "position and out_position: both or neither");
  MS_CHECK_ARG((log_scaling == nullptr) == (out_log_scaling == nullptr), "log_scaling and out_log_scaling: both or neither");
  MS_CHECK_ARG((rotation == nullptr) == (out_rotation == nullptr), "rotation and out_rotation: both or neither");
  MS_CHECK_ARG((feature == nullptr) == (out_feature == nullptr), "feature and out_feature: both or neither");
  if (feature) {
    if (sh_degree < 1 || sh_degree > 3) {
      set_error("ms_scene_transform: sh_degree must be 1..3 when a feature is given (got %d)", sh_degree);
      return MS_ERR_BAD_ARG;
    }
    if (f < 1 || f > (1 << 20)) { set_error("ms_scene_transform: 1 <= f <= 2^20 expected (got %d)", f); return MS_ERR_BAD_ARG; }
  }
  MS_CHECK_ARG(transform_host != nullptr, "transform_host is null");
  MS_CHECK_ARG(aligned(dtype == MS_F64 ? 8 : 4, {position, out_position, log_scaling, out_log_scaling, rotation, out_rotation,
                                                 feature, out_feature}), "every pointer must be aligned to its element type");
  if (n == 0 || !(position || log_scaling || rotation || feature)) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MS_F32)
    return scene_transform_typed<float>(position, out_position, log_scaling, out_log_scaling, rotation, out_rotation,
                                        feature, out_feature, n, f, sh_degree, transform_host, s);
  return scene_transform_typed<double>(position, out_position, log_scaling, out_log_scaling, rotation, out_rotation,
                                       feature, out_feature, n, f, sh_degree, transform_host, s);
}
