// geometry.hip — what a surface-aware trainer needs beside the colour image: a unit normal per gaussian, and the
// consistency of the blended normals with the normals of the blended depth.  The reference has neither.
//
// Per-gaussian normal (ms_gaussian_normals_fwd / _bwd), one lane per gaussian: the shortest axis of the gaussian turned
// to face the camera.  q = rotation / |rotation| (xyzw), k = index of the smallest log_scaling (a tie takes the lowest
// index), n = column k of R(q), negated where n . (position - camera_position) > 0 (exactly 0 keeps the sign).  The forward
// also writes one byte per row, k | flipped << 2: k and the sign are piecewise constant, so the backward reads that byte
// and the quaternion and never repeats the two comparisons (a second evaluation that rounds differently could not then
// disagree with the forward).  The only gradient is to the unnormalised quaternion.
//
// Normal consistency (ms_normal_consistency_fwd / _bwd) on an accumulated (H, W, F) feature image with channels
// depth_sum (oz), alpha (oa) and normal_sum (on, on + 1, on + 2), pixel centre (x + 0.5, y + 0.5):
//   d = depth_sum / alpha                 P = d ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1)
//   a = P(x + 1, y) - P(x - 1, y)         b = P(x, y + 1) - P(x, y - 1)         c = b x a
//   n_d = c / |c| where |c|^2 >= TINY, else 0;   n^ = normal_sum / |normal_sum| under the same rule
//   loss = sum over interior pixels of  w (1 - n^ . n_d) / ((H - 2)(W - 2))
// with w = pixel_weight or alpha (a constant either way) where the pixel and its four neighbours have alpha >= alpha_min,
// else 0.  A workgroup (4 waves) owns 64 x 16 pixels; a lane owns a column and four rows of it.  The forward stages d and
// the alpha test of tile + 1 in LDS.  The backward is ONE launch in gather form: the centre of a stencil is not among its
// own inputs, so d(q) is reached from the four centres next to q, each of which reads its own four neighbours: a
// radius-2 diamond around q.  The workgroup stages d of tile + 2, evaluates dL/dc of the (64 + 2) x (16 + 2) centres of
// tile + 1 into LDS (the ring is evaluated by the neighbouring workgroup as well, with the same instructions), and every
// pixel then gathers  dL/dP(q) = ga(left) - ga(right) + gb(up) - gb(down),  ga = gc x b,  gb = a x gc.  No atomics.
// The loss is one double per workgroup (lane sums -> wave butterfly -> four waves in wave order) added in a fixed order by
// a second one-workgroup kernel: bitwise reproducible.  projection (fx, fy, cx, cy) and the upstream gradient are read
// from device memory: nothing here reads back to the host, and a captured graph follows a camera that changes in place.
#include <math.h>

#include "common.h"

namespace ms {

constexpr int GN_THREADS = 256;
constexpr int NC_TW = 64, NC_TH = 16, NC_WAVES = 4, NC_THREADS = NC_TW * NC_WAVES;
constexpr int NC_ROWS = NC_TH / NC_WAVES;                 // rows of a tile column per lane
constexpr double NC_TINY = MS_NORMAL_TINY;

template <typename T> __device__ __forceinline__ T geo_sqrt(T v);
template <> __device__ __forceinline__ float geo_sqrt(float v) { return sqrtf(v); }
template <> __device__ __forceinline__ double geo_sqrt(double v) { return sqrt(v); }

// ---- per-gaussian normals ---------------------------------------------------------------------------------------------

// column k of R(q) for a unit quaternion (xyzw): quat_to_mat of splat_math.h, one column
template <typename T>
__device__ __forceinline__ void quat_column(T x, T y, T z, T w, int k, T col[3]) {
  if (k == 0) {
    col[0] = 1 - 2 * y * y - 2 * z * z; col[1] = 2 * x * y + 2 * w * z; col[2] = 2 * x * z - 2 * w * y;
  } else if (k == 1) {
    col[0] = 2 * x * y - 2 * w * z; col[1] = 1 - 2 * x * x - 2 * z * z; col[2] = 2 * y * z + 2 * w * x;
  } else {
    col[0] = 2 * x * z + 2 * w * y; col[1] = 2 * y * z - 2 * w * x; col[2] = 1 - 2 * x * x - 2 * y * y;
  }
}

template <typename T>
__global__ void __launch_bounds__(GN_THREADS)
gaussian_normals_fwd_kernel(const T* __restrict__ position, const T* __restrict__ log_scaling,
                            const T* __restrict__ rotation, const T* __restrict__ camera_position, int64_t n,
                            T* __restrict__ normals, uint8_t* __restrict__ code) {
  const int64_t i = (int64_t)blockIdx.x * GN_THREADS + threadIdx.x;
  if (i >= n) return;
  const T qx = rotation[4 * i], qy = rotation[4 * i + 1], qz = rotation[4 * i + 2], qw = rotation[4 * i + 3];
  const T qn = geo_sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
  const T s0 = log_scaling[3 * i], s1 = log_scaling[3 * i + 1], s2 = log_scaling[3 * i + 2];
  int k = 0;
  T smallest = s0;
  if (s1 < smallest) { k = 1; smallest = s1; }
  if (s2 < smallest) k = 2;
  T col[3];
  quat_column(qx / qn, qy / qn, qz / qn, qw / qn, k, col);
  const T dx = position[3 * i] - camera_position[0], dy = position[3 * i + 1] - camera_position[1],
          dz = position[3 * i + 2] - camera_position[2];
  const bool flip = col[0] * dx + col[1] * dy + col[2] * dz > T(0);
  normals[3 * i] = flip ? -col[0] : col[0];
  normals[3 * i + 1] = flip ? -col[1] : col[1];
  normals[3 * i + 2] = flip ? -col[2] : col[2];
  code[i] = (uint8_t)(k | (flip ? 4 : 0));
}

template <typename T>
__global__ void __launch_bounds__(GN_THREADS)
gaussian_normals_bwd_kernel(const T* __restrict__ rotation, const uint8_t* __restrict__ code,
                            const T* __restrict__ grad_normals, int64_t n, T* __restrict__ grad_rotation) {
  const int64_t i = (int64_t)blockIdx.x * GN_THREADS + threadIdx.x;
  if (i >= n) return;
  const T qx = rotation[4 * i], qy = rotation[4 * i + 1], qz = rotation[4 * i + 2], qw = rotation[4 * i + 3];
  const T qn = geo_sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
  const T x = qx / qn, y = qy / qn, z = qz / qn, w = qw / qn;
  const int c = code[i], k = c & 3;
  const T sign = (c & 4) ? T(-1) : T(1);
  const T g0 = sign * grad_normals[3 * i], g1 = sign * grad_normals[3 * i + 1], g2 = sign * grad_normals[3 * i + 2];
  T d[4];                                                 // d / d(unit quaternion) of column k . g
  if (k == 0) {
    d[0] = 2 * (y * g1 + z * g2);
    d[1] = 2 * (-2 * y * g0 + x * g1 - w * g2);
    d[2] = 2 * (-2 * z * g0 + w * g1 + x * g2);
    d[3] = 2 * (z * g1 - y * g2);
  } else if (k == 1) {
    d[0] = 2 * (y * g0 - 2 * x * g1 + w * g2);
    d[1] = 2 * (x * g0 + z * g2);
    d[2] = 2 * (-w * g0 - 2 * z * g1 + y * g2);
    d[3] = 2 * (-z * g0 + x * g2);
  } else {
    d[0] = 2 * (z * g0 - w * g1 - 2 * x * g2);
    d[1] = 2 * (w * g0 + z * g1 - 2 * y * g2);
    d[2] = 2 * (x * g0 + y * g1);
    d[3] = 2 * (y * g0 - x * g1);
  }
  const T qdot = x * d[0] + y * d[1] + z * d[2] + w * d[3];       // through q / |q|, as project_backward does
  grad_rotation[4 * i] = (d[0] - x * qdot) / qn;
  grad_rotation[4 * i + 1] = (d[1] - y * qdot) / qn;
  grad_rotation[4 * i + 2] = (d[2] - z * qdot) / qn;
  grad_rotation[4 * i + 3] = (d[3] - w * qdot) / qn;
}

// ---- normal consistency -----------------------------------------------------------------------------------------------

struct NcDims {
  int H, W, F, oz, oa, on;
};

// d and the alpha test of the tile and `halo` pixels around it; outside the image, and where alpha < alpha_min, d = 0 and
// the test fails (d is never evaluated there)
template <typename T, int HALO>
__device__ __forceinline__ void nc_stage(T (*sd)[NC_TW + 2 * HALO], uint8_t (*sok)[NC_TW + 2 * HALO],
                                         const T* __restrict__ accum, const NcDims& dm, int x0, int y0, T alpha_min) {
  constexpr int LW = NC_TW + 2 * HALO, LR = NC_TH + 2 * HALO;
  for (int idx = threadIdx.x; idx < LR * LW; idx += NC_THREADS) {
    const int r = idx / LW, c = idx - r * LW;
    const int y = y0 - HALO + r, x = x0 - HALO + c;
    T d = T(0);
    uint8_t ok = 0;
    if (x >= 0 && x < dm.W && y >= 0 && y < dm.H) {
      const T* __restrict__ p = accum + ((int64_t)y * dm.W + x) * dm.F;
      const T alpha = p[dm.oa];
      if (alpha >= alpha_min) { ok = 1; d = p[dm.oz] / alpha; }
    }
    sd[r][c] = d;
    sok[r][c] = ok;
  }
}

template <typename T> struct NcCamera { T fx, fy, cx, cy; };

template <typename T>
__device__ __forceinline__ NcCamera<T> nc_camera(const T* __restrict__ projection) {
  return NcCamera<T>{projection[0], projection[1], projection[2], projection[3]};
}

// a = P(x + 1, y) - P(x - 1, y) and b = P(x, y + 1) - P(x, y - 1) from the four staged depths around a centre
template <typename T>
__device__ __forceinline__ void nc_edges(const NcCamera<T>& cam, int x, int y, T dl, T dr, T du, T dd, T a[3], T b[3]) {
  const T ul = (T(x - 1) + T(0.5) - cam.cx) / cam.fx, ur = (T(x + 1) + T(0.5) - cam.cx) / cam.fx;
  const T uc = (T(x) + T(0.5) - cam.cx) / cam.fx;
  const T vu = (T(y - 1) + T(0.5) - cam.cy) / cam.fy, vd = (T(y + 1) + T(0.5) - cam.cy) / cam.fy;
  const T vc = (T(y) + T(0.5) - cam.cy) / cam.fy;
  a[0] = dr * ur - dl * ul; a[1] = dr * vc - dl * vc; a[2] = dr - dl;
  b[0] = dd * uc - du * uc; b[1] = dd * vd - du * vu; b[2] = dd - du;
}

template <typename T>
__device__ __forceinline__ void nc_cross(const T u[3], const T v[3], T out[3]) {
  out[0] = u[1] * v[2] - u[2] * v[1];
  out[1] = u[2] * v[0] - u[0] * v[2];
  out[2] = u[0] * v[1] - u[1] * v[0];
}

// v / |v| where |v|^2 >= TINY (returns 1 / |v|), else 0 (returns 0)
template <typename T>
__device__ __forceinline__ T nc_unit(const T v[3], T out[3]) {
  const T vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
  if (!(vv >= T(NC_TINY))) { out[0] = out[1] = out[2] = T(0); return T(0); }
  const T inv = T(1) / geo_sqrt(vv);
  out[0] = v[0] * inv; out[1] = v[1] * inv; out[2] = v[2] * inv;
  return inv;
}

template <typename T>
__global__ void __launch_bounds__(NC_THREADS)
normal_consistency_fwd_kernel(const T* __restrict__ accum, const T* __restrict__ pixel_weight,
                              const T* __restrict__ projection, NcDims dm, T alpha_min, double* __restrict__ partials,
                              T* __restrict__ depth_normals) {
  __shared__ T sd[NC_TH + 2][NC_TW + 2];
  __shared__ uint8_t sok[NC_TH + 2][NC_TW + 2];
  __shared__ double red[NC_WAVES];
  const int x0 = blockIdx.x * NC_TW, y0 = blockIdx.y * NC_TH;
  nc_stage<T, 1>(sd, sok, accum, dm, x0, y0, alpha_min);
  __syncthreads();
  const NcCamera<T> cam = nc_camera(projection);
  const int col = threadIdx.x & (NC_TW - 1), wave = threadIdx.x / NC_TW;
  const int x = x0 + col;
  double sum = 0.0;                       // a lane's four terms, added in double: only the terms carry the format's error
#pragma unroll
  for (int j = 0; j < NC_ROWS; ++j) {
    const int row = wave * NC_ROWS + j, y = y0 + row;
    if (x >= dm.W || y >= dm.H) continue;
    const int r = row + 1, c = col + 1;
    T nd[3] = {T(0), T(0), T(0)};
    const bool interior = x >= 1 && x <= dm.W - 2 && y >= 1 && y <= dm.H - 2;
    if (interior && sok[r][c] && sok[r][c - 1] && sok[r][c + 1] && sok[r - 1][c] && sok[r + 1][c]) {
      T a[3], b[3], cr[3];
      nc_edges(cam, x, y, sd[r][c - 1], sd[r][c + 1], sd[r - 1][c], sd[r + 1][c], a, b);
      nc_cross(b, a, cr);
      nc_unit(cr, nd);
      const T* __restrict__ p = accum + ((int64_t)y * dm.W + x) * dm.F;
      const T m[3] = {p[dm.on], p[dm.on + 1], p[dm.on + 2]};
      T nh[3];
      nc_unit(m, nh);
      const T w = pixel_weight ? pixel_weight[(int64_t)y * dm.W + x] : p[dm.oa];
      sum += (double)(w * (T(1) - (nh[0] * nd[0] + nh[1] * nd[1] + nh[2] * nd[2])));
    }
    if (depth_normals) {
      T* __restrict__ o = depth_normals + ((int64_t)y * dm.W + x) * 3;
      o[0] = nd[0]; o[1] = nd[1]; o[2] = nd[2];
    }
  }
  sum = wave_sum_to_lane63(sum);
  if (lane_id() == 63) red[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int g = 0; g < NC_WAVES; ++g) t += red[g];
    partials[blockIdx.y * gridDim.x + blockIdx.x] = t;
  }
}

// one workgroup: lane sums over a fixed stride, then a tree over the 256 lanes, all in double
template <typename T>
__global__ void __launch_bounds__(NC_THREADS)
normal_consistency_finalize_kernel(const double* __restrict__ partials, int count, double inv_pixels, T* __restrict__ out) {
  __shared__ double red[NC_THREADS];
  double t = 0.0;
  for (int i = threadIdx.x; i < count; i += NC_THREADS) t += partials[i];
  red[threadIdx.x] = t;
  __syncthreads();
  for (int half = NC_THREADS / 2; half >= 1; half >>= 1) {
    if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (T)(red[0] * inv_pixels);
}

template <typename T>
__global__ void __launch_bounds__(NC_THREADS)
normal_consistency_bwd_kernel(const T* __restrict__ accum, const T* __restrict__ pixel_weight,
                              const T* __restrict__ projection, const T* __restrict__ grad_loss, NcDims dm, T alpha_min,
                              double inv_pixels, T* __restrict__ grad_accum) {
  __shared__ T sd[NC_TH + 4][NC_TW + 4];
  __shared__ uint8_t sok[NC_TH + 4][NC_TW + 4];
  __shared__ T sg[3][NC_TH + 2][NC_TW + 2];               // dL/dc of the centres of tile + 1
  const int x0 = blockIdx.x * NC_TW, y0 = blockIdx.y * NC_TH;
  nc_stage<T, 2>(sd, sok, accum, dm, x0, y0, alpha_min);
  __syncthreads();
  const NcCamera<T> cam = nc_camera(projection);
  const T scale = grad_loss[0] * (T)inv_pixels;

  // centres of tile + 1: dL/dc into LDS; a centre of the tile itself also owns its pixel's normal_sum gradient
  constexpr int CW = NC_TW + 2, CR = NC_TH + 2;
  for (int idx = threadIdx.x; idx < CR * CW; idx += NC_THREADS) {
    const int rc = idx / CW, cc = idx - rc * CW;
    const int y = y0 - 1 + rc, x = x0 - 1 + cc;
    const int r = rc + 1, c = cc + 1;                     // the centre in sd
    T gc[3] = {T(0), T(0), T(0)}, gm[3] = {T(0), T(0), T(0)};
    const bool interior = x >= 1 && x <= dm.W - 2 && y >= 1 && y <= dm.H - 2;
    if (interior && sok[r][c] && sok[r][c - 1] && sok[r][c + 1] && sok[r - 1][c] && sok[r + 1][c]) {
      T a[3], b[3], cr[3], nd[3], nh[3];
      nc_edges(cam, x, y, sd[r][c - 1], sd[r][c + 1], sd[r - 1][c], sd[r + 1][c], a, b);
      nc_cross(b, a, cr);
      const T inv_c = nc_unit(cr, nd);
      const T* __restrict__ p = accum + ((int64_t)y * dm.W + x) * dm.F;
      const T m[3] = {p[dm.on], p[dm.on + 1], p[dm.on + 2]};
      const T inv_m = nc_unit(m, nh);
      const T w = pixel_weight ? pixel_weight[(int64_t)y * dm.W + x] : p[dm.oa];
      const T ws = -(w * scale);                          // d(w (1 - n^ . n_d) scale) / d(n^ . n_d)
      // through v / |v|: (I - n n^T) g / |v|; a vector under TINY is a constant 0 (inv = 0)
      const T dot = nh[0] * nd[0] + nh[1] * nd[1] + nh[2] * nd[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        gc[k] = ws * (nh[k] - nd[k] * dot) * inv_c;
        gm[k] = ws * (nd[k] - nh[k] * dot) * inv_m;
      }
    }
    sg[0][rc][cc] = gc[0]; sg[1][rc][cc] = gc[1]; sg[2][rc][cc] = gc[2];
    if (rc >= 1 && rc <= NC_TH && cc >= 1 && cc <= NC_TW && x < dm.W && y < dm.H) {
      T* __restrict__ o = grad_accum + ((int64_t)y * dm.W + x) * dm.F + dm.on;
      o[0] = gm[0]; o[1] = gm[1]; o[2] = gm[2];
    }
  }
  __syncthreads();

  const int col = threadIdx.x & (NC_TW - 1), wave = threadIdx.x / NC_TW;
  const int x = x0 + col;
#pragma unroll
  for (int j = 0; j < NC_ROWS; ++j) {
    const int row = wave * NC_ROWS + j, y = y0 + row;
    if (x >= dm.W || y >= dm.H) continue;
    const int r = row + 2, c = col + 2;                   // the pixel in sd; in sg it is [row + 1][col + 1]
    T gp[3] = {T(0), T(0), T(0)};
    // the four centres whose stencil holds this pixel: (dx, dy) from the pixel to the centre
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int dx = s == 0 ? -1 : s == 1 ? 1 : 0, dy = s == 2 ? -1 : s == 3 ? 1 : 0;
      const int rc = row + 1 + dy, cc = col + 1 + dx;
      const T gc[3] = {sg[0][rc][cc], sg[1][rc][cc], sg[2][rc][cc]};
      const int pr = r + dy, pc = c + dx;
      T a[3], b[3], t[3];
      nc_edges(cam, x + dx, y + dy, sd[pr][pc - 1], sd[pr][pc + 1], sd[pr - 1][pc], sd[pr + 1][pc], a, b);
      if (dy == 0) nc_cross(gc, b, t);                    // ga = gc x b: the pixel is the centre's x + 1 (dx = -1) or x - 1
      else nc_cross(a, gc, t);                            // gb = a x gc: the pixel is the centre's y + 1 (dy = -1) or y - 1
      const T sgn = (dx + dy) < 0 ? T(1) : T(-1);
      gp[0] += sgn * t[0]; gp[1] += sgn * t[1]; gp[2] += sgn * t[2];
    }
    const T u = (T(x) + T(0.5) - cam.cx) / cam.fx, v = (T(y) + T(0.5) - cam.cy) / cam.fy;
    const T gd = gp[0] * u + gp[1] * v + gp[2];
    T* __restrict__ o = grad_accum + ((int64_t)y * dm.W + x) * dm.F;
    T g_sum = T(0), g_alpha = T(0);
    if (sok[r][c]) {                                      // elsewhere no stencil reads this pixel's depth
      const T alpha = accum[((int64_t)y * dm.W + x) * dm.F + dm.oa];
      g_sum = gd / alpha;
      g_alpha = -(gd * sd[r][c]) / alpha;
    }
    for (int ch = 0; ch < dm.F; ++ch) {
      if (ch >= dm.on && ch < dm.on + 3) continue;        // written above
      o[ch] = ch == dm.oz ? g_sum : ch == dm.oa ? g_alpha : T(0);
    }
  }
}

template <typename T>
static void nc_fwd(const void* accum, const void* pixel_weight, const void* projection, const NcDims& dm, double alpha_min,
                   double* partials, void* out_loss, void* depth_normals, hipStream_t s) {
  const dim3 grid((unsigned)div_up(dm.W, NC_TW), (unsigned)div_up(dm.H, NC_TH));
  const double inv_pixels = dm.H >= 3 && dm.W >= 3 ? 1.0 / ((double)(dm.H - 2) * (double)(dm.W - 2)) : 0.0;
  normal_consistency_fwd_kernel<T><<<grid, dim3(NC_THREADS), 0, s>>>(
      (const T*)accum, (const T*)pixel_weight, (const T*)projection, dm, (T)alpha_min, partials, (T*)depth_normals);
  normal_consistency_finalize_kernel<T><<<dim3(1), dim3(NC_THREADS), 0, s>>>(partials, (int)(grid.x * grid.y), inv_pixels,
                                                                             (T*)out_loss);
}

template <typename T>
static void nc_bwd(const void* accum, const void* pixel_weight, const void* projection, const void* grad_loss,
                   const NcDims& dm, double alpha_min, void* grad_accum, hipStream_t s) {
  const dim3 grid((unsigned)div_up(dm.W, NC_TW), (unsigned)div_up(dm.H, NC_TH));
  const double inv_pixels = dm.H >= 3 && dm.W >= 3 ? 1.0 / ((double)(dm.H - 2) * (double)(dm.W - 2)) : 0.0;
  normal_consistency_bwd_kernel<T><<<grid, dim3(NC_THREADS), 0, s>>>(
      (const T*)accum, (const T*)pixel_weight, (const T*)projection, (const T*)grad_loss, dm, (T)alpha_min, inv_pixels,
      (T*)grad_accum);
}

}  // namespace ms

using namespace ms;

static int gn_check(int64_t n, int dtype, const char* who) {
  if (n < 0) { set_error("%s: n >= 0 expected (got %lld)", who, (long long)n); return MS_ERR_BAD_ARG; }
  if (n > (int64_t)INT32_MAX * GN_THREADS) { set_error("%s: too many rows (%lld)", who, (long long)n); return MS_ERR_UNSUPPORTED; }
  if (dtype != MS_F32 && dtype != MS_F64) { set_error("%s: unknown dtype %d", who, dtype); return MS_ERR_UNSUPPORTED; }
  return 0;
}

extern "C" int ms_gaussian_normals_fwd(const void* position, const void* log_scaling, const void* rotation,
                                       const void* camera_position, int64_t n, int dtype, void* normals, void* code,
                                       void* stream) {
  const int rc = gn_check(n, dtype, "ms_gaussian_normals_fwd");
  if (rc) return rc;
  if (n == 0) return 0;
  MS_CHECK_ARG(position && log_scaling && rotation && camera_position && normals && code, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)div_up(n, GN_THREADS));
  if (dtype == MS_F32)
    gaussian_normals_fwd_kernel<float><<<grid, dim3(GN_THREADS), 0, s>>>(
        (const float*)position, (const float*)log_scaling, (const float*)rotation, (const float*)camera_position, n,
        (float*)normals, (uint8_t*)code);
  else
    gaussian_normals_fwd_kernel<double><<<grid, dim3(GN_THREADS), 0, s>>>(
        (const double*)position, (const double*)log_scaling, (const double*)rotation, (const double*)camera_position, n,
        (double*)normals, (uint8_t*)code);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_gaussian_normals_bwd(const void* rotation, const void* code, const void* grad_normals, int64_t n,
                                       int dtype, void* grad_rotation, void* stream) {
  const int rc = gn_check(n, dtype, "ms_gaussian_normals_bwd");
  if (rc) return rc;
  if (n == 0) return 0;
  MS_CHECK_ARG(rotation && code && grad_normals && grad_rotation, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)div_up(n, GN_THREADS));
  if (dtype == MS_F32)
    gaussian_normals_bwd_kernel<float><<<grid, dim3(GN_THREADS), 0, s>>>(
        (const float*)rotation, (const uint8_t*)code, (const float*)grad_normals, n, (float*)grad_rotation);
  else
    gaussian_normals_bwd_kernel<double><<<grid, dim3(GN_THREADS), 0, s>>>(
        (const double*)rotation, (const uint8_t*)code, (const double*)grad_normals, n, (double*)grad_rotation);
  MS_CHECK_LAUNCH();
  return 0;
}

static int nc_check(int H, int W, int F, int oz, int oa, int on, int dtype, double alpha_min, const char* who) {
  if (H <= 0 || W <= 0) { set_error("%s: H, W > 0 expected (got %d x %d)", who, H, W); return MS_ERR_BAD_ARG; }
  if (F < 5) { set_error("%s: F >= 5 channels expected (depth, alpha and three of the normal; got %d)", who, F); return MS_ERR_BAD_ARG; }
  if (oz < 0 || oz >= F || oa < 0 || oa >= F || on < 0 || on + 3 > F) {
    set_error("%s: channel offsets (%d, %d, %d) outside 0..%d", who, oz, oa, on, F - 1);
    return MS_ERR_BAD_ARG;
  }
  if (oz == oa || (oz >= on && oz < on + 3) || (oa >= on && oa < on + 3)) {
    set_error("%s: channel offsets (%d, %d, %d..%d) overlap", who, oz, oa, on, on + 2);
    return MS_ERR_BAD_ARG;
  }
  if (!(alpha_min > 0.0)) { set_error("%s: alpha_min > 0 expected (got %g)", who, alpha_min); return MS_ERR_BAD_ARG; }
  if ((int64_t)H * W * F > INT32_MAX) { set_error("%s: image too large (%d x %d x %d)", who, H, W, F); return MS_ERR_UNSUPPORTED; }
  if (dtype != MS_F32 && dtype != MS_F64) { set_error("%s: unknown dtype %d", who, dtype); return MS_ERR_UNSUPPORTED; }
  return 0;
}

extern "C" int ms_normal_consistency_fwd(const void* accum, const void* pixel_weight, const void* projection, int H, int W,
                                         int F, int depth_offset, int alpha_offset, int normal_offset, int dtype,
                                         double alpha_min, void* tmp, size_t* tmp_bytes, void* out_loss,
                                         void* depth_normals, void* stream) {
  const int rc = nc_check(H, W, F, depth_offset, alpha_offset, normal_offset, dtype, alpha_min, "ms_normal_consistency_fwd");
  if (rc) return rc;
  MS_CHECK_TMP(tmp, tmp_bytes, Carve::one((size_t)(div_up(W, NC_TW) * div_up(H, NC_TH)) * sizeof(double)));
  MS_CHECK_ARG(accum && projection && out_loss, "null pointer");
  const NcDims dm{H, W, F, depth_offset, alpha_offset, normal_offset};
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MS_F32) nc_fwd<float>(accum, pixel_weight, projection, dm, alpha_min, (double*)tmp, out_loss, depth_normals, s);
  else nc_fwd<double>(accum, pixel_weight, projection, dm, alpha_min, (double*)tmp, out_loss, depth_normals, s);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_normal_consistency_bwd(const void* accum, const void* pixel_weight, const void* projection,
                                         const void* grad_loss, int H, int W, int F, int depth_offset, int alpha_offset,
                                         int normal_offset, int dtype, double alpha_min, void* grad_accum, void* stream) {
  const int rc = nc_check(H, W, F, depth_offset, alpha_offset, normal_offset, dtype, alpha_min, "ms_normal_consistency_bwd");
  if (rc) return rc;
  MS_CHECK_ARG(accum && projection && grad_loss && grad_accum, "null pointer");
  const NcDims dm{H, W, F, depth_offset, alpha_offset, normal_offset};
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MS_F32) nc_bwd<float>(accum, pixel_weight, projection, grad_loss, dm, alpha_min, grad_accum, s);
  else nc_bwd<double>(accum, pixel_weight, projection, grad_loss, dm, alpha_min, grad_accum, s);
  MS_CHECK_LAUNCH();
  return 0;
}
