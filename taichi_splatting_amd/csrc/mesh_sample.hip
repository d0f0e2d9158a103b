// mesh_sample.hip — uniform, area-weighted, stratified, seeded samples of a triangle mesh's surface: what a mesh is
// turned into before it is scored against a ground-truth cloud (Chamfer distance, precision / recall / F-score:
// taichi_splatting_amd/mesh_eval.py).  Kernels of this file = 2.
//
//   mesh_face_areas_kernel     one lane per face: area = 0.5 |(b - a) x (c - a)|, differences, products and the sum of
//                              squares ((x x + y y) + z z) in float64 on the float32 positions, unfused.  A face with an
//                              index outside 0 .. V - 1 or a referenced vertex that is not finite sets MS_MESH_BAD_INDEX
//                              / MS_MESH_NOT_FINITE in the status word (an integer OR: no order shows) and gets area 0.
//                              The caller turns the areas into an inclusive float64 cdf (a cumulative sum).
//   mesh_sample_points_kernel  one lane per sample i of n:
//                                t    = min((i + u0) (cdf[T - 1] / n), nextafter(cdf[T - 1], 0))        float64
//                                face = the first f with cdf[f] > t (binary search): a face of area 0 is never drawn
//                                r    = sqrt(u1), (wa, wb, wc) = (1 - r, r (1 - u2), r u2)              float32
//                                p    = (wa A + wb B) + wc C per component, float32, unfused
//                              colours and normals are the same combination of the three vertex rows (normals not
//                              renormalised); without vertex normals, out_normals is the unit face normal
//                              (b - a) x (c - a) / |.| in float64, rounded once.
//
// RANDOM NUMBERS are counter-based: a function of (seed, i, j) and of no state.
//   mix(x):          x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16          (uint32)
//   word(seed, i, j) = mix((uint32)i + mix((uint32)seed + 0x9e3779b9 (j + 1)))
//   u_j              = (word(seed, i, j) >> 8) 2^-24                         j = 0, 1, 2: 24 bits, exact in float32
// No atomics on data, no LDS, no host read: two calls give equal bits.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace ms {

__device__ __forceinline__ uint32_t sample_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

__device__ __forceinline__ uint32_t sample_word(uint32_t seed, uint32_t i, uint32_t j) {
  return sample_mix(i + sample_mix(seed + 0x9e3779b9u * (j + 1u)));
}

__device__ __forceinline__ float sample_unit(uint32_t seed, uint32_t i, uint32_t j) {
  return (float)(sample_word(seed, i, j) >> 8) * 0x1p-24f;
}

__device__ __forceinline__ bool sample_finite3(const float* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// (b - a) x (c - a) in float64 on the float32 positions
__device__ __forceinline__ void sample_cross(const float* a, const float* b, const float* c, double out[3]) {
  const double ux = (double)b[0] - (double)a[0], uy = (double)b[1] - (double)a[1], uz = (double)b[2] - (double)a[2];
  const double wx = (double)c[0] - (double)a[0], wy = (double)c[1] - (double)a[1], wz = (double)c[2] - (double)a[2];
  out[0] = uy * wz - uz * wy;
  out[1] = uz * wx - ux * wz;
  out[2] = ux * wy - uy * wx;
}

__global__ void __launch_bounds__(256)
mesh_face_areas_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int num_vertices,
                       int num_faces, double* __restrict__ area, int32_t* __restrict__ status) {
  const int64_t f = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
  if (f >= num_faces) return;
  const int ia = faces[3 * f + 0], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  if ((unsigned)ia >= (unsigned)num_vertices || (unsigned)ib >= (unsigned)num_vertices || (unsigned)ic >= (unsigned)num_vertices) {
    atomicOr(status, MS_MESH_BAD_INDEX);
    area[f] = 0.0;
    return;
  }
  const float* a = vertices + (int64_t)ia * 3;
  const float* b = vertices + (int64_t)ib * 3;
  const float* c = vertices + (int64_t)ic * 3;
  if (!(sample_finite3(a) && sample_finite3(b) && sample_finite3(c))) {
    atomicOr(status, MS_MESH_NOT_FINITE);
    area[f] = 0.0;
    return;
  }
  double m[3];
  sample_cross(a, b, c, m);
  area[f] = 0.5 * sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
}

__device__ __forceinline__ void sample_combine(const float* __restrict__ rows, int ia, int ib, int ic, float wa, float wb,
                                               float wc, float* __restrict__ out) {
#pragma unroll
  for (int k = 0; k < 3; ++k)
    out[k] = (wa * rows[(int64_t)ia * 3 + k] + wb * rows[(int64_t)ib * 3 + k]) + wc * rows[(int64_t)ic * 3 + k];
}

__global__ void __launch_bounds__(256)
mesh_sample_points_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                          const float* __restrict__ colours, const float* __restrict__ normals, int num_vertices,
                          int num_faces, const double* __restrict__ cdf, int n, uint32_t seed,
                          float* __restrict__ out_points, int32_t* __restrict__ out_face, float* __restrict__ out_bary,
                          float* __restrict__ out_colours, float* __restrict__ out_normals) {
  const int64_t i = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
  if (i >= n) return;
  const float u0 = sample_unit(seed, (uint32_t)i, 0), u1 = sample_unit(seed, (uint32_t)i, 1), u2 = sample_unit(seed, (uint32_t)i, 2);

  const double total = cdf[num_faces - 1];
  const double below = total > 0.0 ? __longlong_as_double(__double_as_longlong(total) - 1) : total;    // nextafter(total, 0)
  const double t = fmin(((double)i + (double)u0) * (total / (double)n), below);
  int lo = 0, hi = num_faces - 1;          // the first f with cdf[f] > t; cdf[T - 1] > t, so the answer is <= T - 1
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (cdf[mid] > t) hi = mid; else lo = mid + 1;
  }
  const int f = lo;
  // the areas call gave a face with a bad index the area 0, so it is not drawn; clamped all the same: no stray access
  const int ia = min(max(faces[3 * (int64_t)f + 0], 0), num_vertices - 1);
  const int ib = min(max(faces[3 * (int64_t)f + 1], 0), num_vertices - 1);
  const int ic = min(max(faces[3 * (int64_t)f + 2], 0), num_vertices - 1);

  // correctly rounded whatever the compiler's float sqrt is: a float64 square root of a float32 value, rounded to
  // float32, is the correctly rounded float32 square root (53 >= 2 * 24 + 2 bits)
  const float r = (float)sqrt((double)u1);
  const float wa = 1.0f - r, wb = r * (1.0f - u2), wc = r * u2;
  sample_combine(vertices, ia, ib, ic, wa, wb, wc, out_points + i * 3);
  if (out_face != nullptr) out_face[i] = f;
  if (out_bary != nullptr) {
    out_bary[i * 3 + 0] = wa;
    out_bary[i * 3 + 1] = wb;
    out_bary[i * 3 + 2] = wc;
  }
  if (out_colours != nullptr) sample_combine(colours, ia, ib, ic, wa, wb, wc, out_colours + i * 3);
  if (out_normals != nullptr) {
    if (normals != nullptr) {
      sample_combine(normals, ia, ib, ic, wa, wb, wc, out_normals + i * 3);
    } else {
      double m[3];
      sample_cross(vertices + (int64_t)ia * 3, vertices + (int64_t)ib * 3, vertices + (int64_t)ic * 3, m);
      const double length = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
      const bool ok = length > 0.0 && isfinite(length);
#pragma unroll
      for (int k = 0; k < 3; ++k) out_normals[i * 3 + k] = ok ? (float)(m[k] / length) : 0.0f;
    }
  }
}

}  // namespace ms

using namespace ms;

extern "C" int ms_mesh_face_areas(const float* vertices, const int32_t* faces, int64_t num_vertices, int64_t num_faces,
                                  double* area, int32_t* status, void* stream) {
  MS_CHECK_ARG(num_vertices >= 0 && num_vertices <= MS_MESH_MAX_VERTICES, "num_vertices outside 0 .. MS_MESH_MAX_VERTICES");
  MS_CHECK_ARG(num_faces >= 0 && 3 * num_faces <= MS_MESH_MAX_CORNERS, "3 num_faces outside 0 .. MS_MESH_MAX_CORNERS");
  MS_CHECK_ARG(status != nullptr, "status is null");
  MS_CHECK_ARG(num_faces == 0 || (faces != nullptr && area != nullptr), "faces or area is null");
  MS_CHECK_ARG(num_vertices == 0 || vertices != nullptr, "vertices is null");
  MS_CHECK_ARG(aligned(4, {vertices, faces, status}) && aligned(8, {area}), "a pointer is not aligned to its element");
  hipStream_t s = (hipStream_t)stream;
  MS_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
  if (num_faces == 0) return 0;
  mesh_face_areas_kernel<<<(unsigned)div_up(num_faces, 256), 256, 0, s>>>(vertices, faces, (int)num_vertices, (int)num_faces,
                                                                         area, status);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_mesh_sample_points(const float* vertices, const int32_t* faces, const float* colours, const float* normals,
                                     int64_t num_vertices, int64_t num_faces, const double* cdf, int64_t n, int64_t seed,
                                     float* out_points, int32_t* out_face, float* out_bary, float* out_colours,
                                     float* out_normals, void* stream) {
  MS_CHECK_ARG(num_vertices >= 0 && num_vertices <= MS_MESH_MAX_VERTICES, "num_vertices outside 0 .. MS_MESH_MAX_VERTICES");
  MS_CHECK_ARG(num_faces >= 0 && 3 * num_faces <= MS_MESH_MAX_CORNERS, "3 num_faces outside 0 .. MS_MESH_MAX_CORNERS");
  MS_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "n outside 0 .. 2^31 - 1");
  if (n == 0) return 0;
  MS_CHECK_ARG(num_vertices >= 1 && num_faces >= 1, "a mesh without a vertex or a face has no surface to sample");
  MS_CHECK_ARG(vertices != nullptr && faces != nullptr && cdf != nullptr && out_points != nullptr,
               "vertices, faces, cdf or out_points is null");
  MS_CHECK_ARG(out_colours == nullptr || colours != nullptr, "out_colours without colours");
  MS_CHECK_ARG(aligned(4, {vertices, faces, colours, normals, out_points, out_face, out_bary, out_colours, out_normals}) &&
                 aligned(8, {cdf}), "a pointer is not aligned to its element");
  mesh_sample_points_kernel<<<(unsigned)div_up(n, 256), 256, 0, (hipStream_t)stream>>>(
    vertices, faces, colours, normals, (int)num_vertices, (int)num_faces, cdf, (int)n, (uint32_t)(uint64_t)seed, out_points,
    out_face, out_bary, out_colours, out_normals);
  MS_CHECK_LAUNCH();
  return 0;
}
