// loss.hip — the photometric loss of a 3-D gaussian-splatting trainer, (1 - lambda) L1 + lambda (1 - SSIM), forward and
// backward on (H, W, C) images as the rasterizer writes and reads them: no permute, no copy.  The reference has no loss
// (its demo calls torch's mse_loss); the torch composition this replaces is a permute to NCHW, five depthwise 11x11
// conv2d, a dozen element-wise kernels and the autograd chain back through all of them.
//
// SSIM per channel, G the separable 11-tap gaussian window (sigma 1.5, normalised), C1 = 0.01^2, C2 = 0.03^2:
//   mu1 = G*x  mu2 = G*y  s11 = G*x^2 - mu1^2  s22 = G*y^2 - mu2^2  s12 = G*xy - mu1 mu2
//   f = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s11 + s22 + C2))
// `same` zero-pads like conv2d(padding = 5); `valid` keeps the (H - 10, W - 10) elements whose window lies inside.
// Both are one code path: a map element is named by the image pixel at its window's CENTRE and exists where that centre
// is at least `margin` (0 | 5) pixels from every border; everything outside the image reads as zero.
//
// Tiling.  An image is H rows of W*C floats, and the horizontal pass is an 11-tap filter of stride C along a row, so a
// tile is cut in FLOATS, not pixels: 64 consecutive floats x TH rows for every C, loads and stores coalesced along W*C.
// A workgroup (4 waves) stages tile + halo (TH + 10 rows of 64 + 10 C floats) of both images in LDS.  A lane owns one
// column; wave g owns rows [g RPT, (g + 1) RPT) of it.  It walks down the RPT + 10 staged rows of its span: the five
// horizontal moments of a row come from LDS (lanes of a wave read consecutive floats of one row: conflict-free whatever
// the row pitch) and are added, with the 11 tap weights, into a rolling window of 11 partial output rows x 5 moments
// (backward: x 3) held in registers: p[j] belongs to the output row whose tap j is the staged row in hand.  After each
// row p[10] is complete; it is evaluated and stored, and the window rolls on by one row.  The vertical pass touches no
// LDS at all, and the walk stays a rolled loop (fully unrolled over per-output accumulators it compiled to 410 VGPRs).
//
// Backward.  With A = df/dmu1 - 2 mu1 df/ds11 - mu2 df/ds12, B = df/ds11, C = df/ds12 saved per map element by the
// forward,  dmean(f)/dx = (G*A + 2 x G*B + y G*C) / N2:  the window is symmetric, so the adjoint of the zero-padded
// filter is the same filter (`valid`: absent map elements read as zero, which is the full correlation).  Three maps
// instead of the five moments: the backward filters three quantities instead of recomputing five and stays one pass.
//
// Reduction.  Each workgroup writes ONE (sum |x - y|, sum f) pair (lane sums -> wave butterfly -> four waves in wave
// order), a second one-workgroup kernel adds the pairs in a fixed order in double: no float atomics, the loss is
// bit-reproducible.  The upstream gradient is read from device memory: nothing here reads back to the host.
#include <math.h>

#include "common.h"

namespace ms {

constexpr int PH_COLS = 64;                // floats per tile row = lanes of a wave
constexpr int PH_GROUPS = 4;               // waves per workgroup, each owns RPT rows of the tile
constexpr int PH_TAPS = 11, PH_R = 5;
constexpr int PH_MAX_C = 4;

template <typename T> struct PhWindow { T g[PH_TAPS]; };

// rows per wave: the float tile is 64 x 32 (LDS 2 x 42 x (64 + 10 C) floats: 31.6 KB at C = 3, five workgroups per CU; 35 KB at C = 4, four),
// the double tile 64 x 16 (the three maps of the backward: 3 x 26 x 104 x 8 bytes < 64 KB)
template <typename T> struct PhRows { static constexpr int value = 8; };
template <> struct PhRows<double> { static constexpr int value = 4; };
template <typename T> __device__ __forceinline__ T ph_abs(T v) { return v < T(0) ? -v : v; }

// tile + halo of one (rows, row_floats) array into LDS; element (i, f) is read at src[(i - margin) * pitch + f - shift]
// where it exists (margin <= i < rows - margin, lo <= f < hi), zero elsewhere
template <typename T, int LR, int LW>
__device__ __forceinline__ void ph_stage(T (*lds)[LW], const T* __restrict__ src, int row0, int f0, int rows, int margin,
                                         int lo, int hi, int64_t pitch, int shift) {
  for (int idx = threadIdx.x; idx < LR * LW; idx += PH_COLS * PH_GROUPS) {
    const int r = idx / LW, c = idx - r * LW;
    const int i = row0 + r, f = f0 + c;
    T v = T(0);
    if (i >= margin && i < rows - margin && f >= lo && f < hi) v = src[(int64_t)(i - margin) * pitch + (f - shift)];
    lds[r][c] = v;
  }
}

template <typename T, int CH>
__global__ void __launch_bounds__(PH_COLS * PH_GROUPS)
photometric_fwd_kernel(const T* __restrict__ x, const T* __restrict__ y, int H, int W, int margin, PhWindow<T> win,
                       T* __restrict__ map_a, T* __restrict__ map_b, T* __restrict__ map_c,
                       double* __restrict__ partials) {
  constexpr int RPT = PhRows<T>::value, TH = RPT * PH_GROUPS;
  constexpr int LR = TH + 2 * PH_R, LW = PH_COLS + 2 * PH_R * CH;
  __shared__ T sx[LR][LW];
  __shared__ T sy[LR][LW];
  __shared__ double red[2 * PH_GROUPS];
  const int WC = W * CH;
  const int f_tile = blockIdx.x * PH_COLS, row_tile = blockIdx.y * TH;
  ph_stage<T, LR, LW>(sx, x, row_tile - PH_R, f_tile - PH_R * CH, H, 0, 0, WC, WC, 0);
  ph_stage<T, LR, LW>(sy, y, row_tile - PH_R, f_tile - PH_R * CH, H, 0, 0, WC, WC, 0);
  __syncthreads();

  const int col = threadIdx.x & (PH_COLS - 1), grp = threadIdx.x / PH_COLS;
  const T c1 = T(0.01 * 0.01), c2 = T(0.03 * 0.03);
  const int f = f_tile + col;
  const int pixel = f / CH;
  const bool col_in_image = f < WC;
  const bool col_in_map = col_in_image && pixel >= margin && pixel < W - margin;
  const int64_t map_pitch = (int64_t)(W - 2 * margin) * CH;
  double sum_l1 = 0.0, sum_f = 0.0;          // a lane's few elements, added in double: only the elements carry float error
  // p[j]: the partial vertical sums of the output row whose tap j is the staged row in hand; p[10] is complete after
  // that row, is evaluated, and the window rolls on by one row
  T p[PH_TAPS][5];
#pragma unroll
  for (int j = 0; j < PH_TAPS; ++j)
#pragma unroll
    for (int m = 0; m < 5; ++m) p[j][m] = T(0);
#pragma unroll 1
  for (int r = 0; r < RPT + 2 * PH_R; ++r) {
    const T* __restrict__ rx = &sx[grp * RPT + r][col];
    const T* __restrict__ ry = &sy[grp * RPT + r][col];
    T h0 = T(0), h1 = T(0), h2 = T(0), h3 = T(0), h4 = T(0);
#pragma unroll
    for (int k = 0; k < PH_TAPS; ++k) {
      const T xv = rx[k * CH], yv = ry[k * CH];
      const T gx = win.g[k] * xv, gy = win.g[k] * yv;
      h0 += gx; h1 += gy;
      h2 += gx * xv; h3 += gy * yv; h4 += gx * yv;
    }
#pragma unroll
    for (int j = 0; j < PH_TAPS; ++j) {
      const T g = win.g[j];
      p[j][0] += g * h0; p[j][1] += g * h1; p[j][2] += g * h2; p[j][3] += g * h3; p[j][4] += g * h4;
    }
    if (r >= 2 * PH_R) {
      const int o = r - 2 * PH_R;
      const int i = row_tile + grp * RPT + o;
      if (i < H && col_in_image) sum_l1 += (double)ph_abs(rx[-PH_R * LW + PH_R * CH] - ry[-PH_R * LW + PH_R * CH]);
      if (i >= margin && i < H - margin && col_in_map) {
        const T mu1 = p[10][0], mu2 = p[10][1];
        const T s11 = p[10][2] - mu1 * mu1, s22 = p[10][3] - mu2 * mu2, s12 = p[10][4] - mu1 * mu2;
        const T a1 = T(2) * mu1 * mu2 + c1, a2 = T(2) * s12 + c2;
        const T b1 = mu1 * mu1 + mu2 * mu2 + c1, b2 = s11 + s22 + c2;
        const T inv = T(1) / (b1 * b2);
        const T fv = a1 * a2 * inv;
        sum_f += (double)fv;
        if (map_a) {
          const T df_dmu1 = T(2) * (mu2 * a2 - mu1 * fv * b2) * inv;     // s11, s22, s12 held fixed
          const T df_ds11 = -fv / b2;
          const T df_ds12 = T(2) * a1 * inv;
          const int64_t at = (int64_t)(i - margin) * map_pitch + (f - margin * CH);
          map_a[at] = df_dmu1 - T(2) * mu1 * df_ds11 - mu2 * df_ds12;
          map_b[at] = df_ds11;
          map_c[at] = df_ds12;
        }
      }
    }
#pragma unroll
    for (int j = PH_TAPS - 1; j > 0; --j)
#pragma unroll
      for (int m = 0; m < 5; ++m) p[j][m] = p[j - 1][m];
#pragma unroll
    for (int m = 0; m < 5; ++m) p[0][m] = T(0);
  }

  // lanes -> wave (butterfly: the same order in every launch) -> the four waves in wave order
  const double w_l1 = wave_sum_to_lane63(sum_l1), w_f = wave_sum_to_lane63(sum_f);
  if (col == PH_COLS - 1) { red[2 * grp] = w_l1; red[2 * grp + 1] = w_f; }
  __syncthreads();
  if (threadIdx.x < 2) {
    double t = 0.0;
    for (int g = 0; g < PH_GROUPS; ++g) t += red[2 * g + threadIdx.x];
    partials[2 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) + threadIdx.x] = t;
  }
}

// out = {loss, l1, ssim}: the workgroup pairs added in a fixed order (lane t takes pairs t, t + 256, ... in order, then
// a fixed tree over the 256 lanes), in double
template <typename T>
__global__ void __launch_bounds__(256)
photometric_finalize_kernel(const double* __restrict__ partials, int64_t count, double n1, double n2, double lambda,
                            T* __restrict__ out) {
  __shared__ double red[2][256];
  double a = 0.0, b = 0.0;
  for (int64_t p = threadIdx.x; p < count; p += 256) { a += partials[2 * p]; b += partials[2 * p + 1]; }
  red[0][threadIdx.x] = a; red[1][threadIdx.x] = b;
  __syncthreads();
  for (int half = 128; half >= 1; half >>= 1) {
    if ((int)threadIdx.x < half) {
      red[0][threadIdx.x] += red[0][threadIdx.x + half];
      red[1][threadIdx.x] += red[1][threadIdx.x + half];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) {
    const double l1 = red[0][0] / n1, ssim = red[1][0] / n2;
    const double loss = (1.0 - lambda) * l1 + lambda * (1.0 - ssim);
    out[threadIdx.x] = (T)(threadIdx.x == 0 ? loss : threadIdx.x == 1 ? l1 : ssim);
  }
}

template <typename T, int CH>
__global__ void __launch_bounds__(PH_COLS * PH_GROUPS)
photometric_bwd_kernel(const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ map_a,
                       const T* __restrict__ map_b, const T* __restrict__ map_c, const T* __restrict__ grad_out,
                       int H, int W, int margin, PhWindow<T> win, T k_l1, T k_ssim, T* __restrict__ grad_x) {
  constexpr int RPT = PhRows<T>::value, TH = RPT * PH_GROUPS;
  constexpr int LR = TH + 2 * PH_R, LW = PH_COLS + 2 * PH_R * CH;
  __shared__ T sa[LR][LW];
  __shared__ T sb[LR][LW];
  __shared__ T sc[LR][LW];
  const int WC = W * CH;
  const int f_tile = blockIdx.x * PH_COLS, row_tile = blockIdx.y * TH;
  const int64_t map_pitch = (int64_t)(W - 2 * margin) * CH;
  const int lo = margin * CH, hi = (W - margin) * CH;
  ph_stage<T, LR, LW>(sa, map_a, row_tile - PH_R, f_tile - PH_R * CH, H, margin, lo, hi, map_pitch, lo);
  ph_stage<T, LR, LW>(sb, map_b, row_tile - PH_R, f_tile - PH_R * CH, H, margin, lo, hi, map_pitch, lo);
  ph_stage<T, LR, LW>(sc, map_c, row_tile - PH_R, f_tile - PH_R * CH, H, margin, lo, hi, map_pitch, lo);
  __syncthreads();

  const int col = threadIdx.x & (PH_COLS - 1), grp = threadIdx.x / PH_COLS;
  const int f = f_tile + col;
  const T go = grad_out[0];
  T p[PH_TAPS][3];
#pragma unroll
  for (int j = 0; j < PH_TAPS; ++j) p[j][0] = p[j][1] = p[j][2] = T(0);
#pragma unroll 1
  for (int r = 0; r < RPT + 2 * PH_R; ++r) {
    const T* __restrict__ ra = &sa[grp * RPT + r][col];
    const T* __restrict__ rb = &sb[grp * RPT + r][col];
    const T* __restrict__ rc = &sc[grp * RPT + r][col];
    T h0 = T(0), h1 = T(0), h2 = T(0);
#pragma unroll
    for (int k = 0; k < PH_TAPS; ++k) {
      h0 += win.g[k] * ra[k * CH]; h1 += win.g[k] * rb[k * CH]; h2 += win.g[k] * rc[k * CH];
    }
#pragma unroll
    for (int j = 0; j < PH_TAPS; ++j) {
      const T g = win.g[j];
      p[j][0] += g * h0; p[j][1] += g * h1; p[j][2] += g * h2;
    }
    const int i = row_tile + grp * RPT + r - 2 * PH_R;
    if (r >= 2 * PH_R && i < H && f < WC) {
      const int64_t at = (int64_t)i * WC + f;
      const T xv = x[at], yv = y[at];
      const T d = xv - yv;
      const T sign = d > T(0) ? T(1) : d < T(0) ? T(-1) : T(0);
      grad_x[at] = go * (k_l1 * sign - k_ssim * (p[10][0] + T(2) * xv * p[10][1] + yv * p[10][2]));
    }
#pragma unroll
    for (int j = PH_TAPS - 1; j > 0; --j) { p[j][0] = p[j - 1][0]; p[j][1] = p[j - 1][1]; p[j][2] = p[j - 1][2]; }
    p[0][0] = p[0][1] = p[0][2] = T(0);
  }
}

template <typename T> static PhWindow<T> ph_window() {
  double g[PH_TAPS], sum = 0.0;
  for (int k = 0; k < PH_TAPS; ++k) { g[k] = exp(-(double)((k - PH_R) * (k - PH_R)) / (2.0 * 1.5 * 1.5)); sum += g[k]; }
  PhWindow<T> w;
  for (int k = 0; k < PH_TAPS; ++k) w.g[k] = (T)(g[k] / sum);
  return w;
}

template <typename T> static dim3 ph_grid(int H, int W, int C) {
  return dim3((unsigned)div_up((int64_t)W * C, PH_COLS), (unsigned)div_up(H, PhRows<T>::value * PH_GROUPS));
}

template <typename T, int CH>
static void ph_launch_fwd(const void* x, const void* y, int H, int W, int margin, void* a, void* b, void* c,
                          double* partials, hipStream_t s) {
  photometric_fwd_kernel<T, CH><<<ph_grid<T>(H, W, CH), dim3(PH_COLS * PH_GROUPS), 0, s>>>(
      (const T*)x, (const T*)y, H, W, margin, ph_window<T>(), (T*)a, (T*)b, (T*)c, partials);
}

template <typename T, int CH>
static void ph_launch_bwd(const void* x, const void* y, const void* a, const void* b, const void* c, const void* go,
                          int H, int W, int margin, double k_l1, double k_ssim, void* grad, hipStream_t s) {
  photometric_bwd_kernel<T, CH><<<ph_grid<T>(H, W, CH), dim3(PH_COLS * PH_GROUPS), 0, s>>>(
      (const T*)x, (const T*)y, (const T*)a, (const T*)b, (const T*)c, (const T*)go, H, W, margin, ph_window<T>(),
      (T)k_l1, (T)k_ssim, (T*)grad);
}

template <typename T>
static void ph_fwd(const void* x, const void* y, int H, int W, int C, int margin, double lambda, void* a, void* b,
                   void* c, double* partials, void* out, hipStream_t s) {
  switch (C) {
    case 1: ph_launch_fwd<T, 1>(x, y, H, W, margin, a, b, c, partials, s); break;
    case 2: ph_launch_fwd<T, 2>(x, y, H, W, margin, a, b, c, partials, s); break;
    case 3: ph_launch_fwd<T, 3>(x, y, H, W, margin, a, b, c, partials, s); break;
    default: ph_launch_fwd<T, 4>(x, y, H, W, margin, a, b, c, partials, s); break;
  }
  const dim3 grid = ph_grid<T>(H, W, C);
  const double n1 = (double)H * W * C, n2 = (double)(H - 2 * margin) * (W - 2 * margin) * C;
  photometric_finalize_kernel<T><<<dim3(1), dim3(256), 0, s>>>(partials, (int64_t)grid.x * grid.y, n1, n2, lambda, (T*)out);
}

template <typename T>
static void ph_bwd(const void* x, const void* y, const void* a, const void* b, const void* c, const void* go, int H,
                   int W, int C, int margin, double lambda, void* grad, hipStream_t s) {
  const double n1 = (double)H * W * C, n2 = (double)(H - 2 * margin) * (W - 2 * margin) * C;
  const double k_l1 = (1.0 - lambda) / n1, k_ssim = lambda / n2;
  switch (C) {
    case 1: ph_launch_bwd<T, 1>(x, y, a, b, c, go, H, W, margin, k_l1, k_ssim, grad, s); break;
    case 2: ph_launch_bwd<T, 2>(x, y, a, b, c, go, H, W, margin, k_l1, k_ssim, grad, s); break;
    case 3: ph_launch_bwd<T, 3>(x, y, a, b, c, go, H, W, margin, k_l1, k_ssim, grad, s); break;
    default: ph_launch_bwd<T, 4>(x, y, a, b, c, go, H, W, margin, k_l1, k_ssim, grad, s); break;
  }
}

}  // namespace ms

using namespace ms;

// sizes, padding and dtype of both entry points; *margin = 0 (same) | 5 (valid)
static int ph_check(int H, int W, int C, int dtype, int padding, const char* who, int* margin) {
  if (H <= 0 || W <= 0) { set_error("%s: H, W > 0 expected (got %d x %d)", who, H, W); return MS_ERR_BAD_ARG; }
  if (C < 1 || C > PH_MAX_C) { set_error("%s: 1 <= C <= %d expected (got %d)", who, PH_MAX_C, C); return MS_ERR_BAD_ARG; }
  if (padding != MS_PAD_SAME && padding != MS_PAD_VALID) {
    set_error("%s: padding must be MS_PAD_SAME or MS_PAD_VALID (got %d)", who, padding);
    return MS_ERR_BAD_ARG;
  }
  if (padding == MS_PAD_VALID && (H < PH_TAPS || W < PH_TAPS)) {
    set_error("%s: valid padding needs H, W >= %d (got %d x %d)", who, PH_TAPS, H, W);
    return MS_ERR_BAD_ARG;
  }
  if ((int64_t)H * W * C > INT32_MAX || div_up(H, 16) > 65535) {
    set_error("%s: image too large (%d x %d x %d)", who, H, W, C);
    return MS_ERR_BAD_ARG;
  }
  if (dtype != MS_F32 && dtype != MS_F64) { set_error("%s: unknown dtype %d", who, dtype); return MS_ERR_UNSUPPORTED; }
  *margin = padding == MS_PAD_VALID ? PH_R : 0;
  return 0;
}

extern "C" int ms_photometric_fwd(const void* image, const void* target, int H, int W, int C, int dtype, int padding,
                                  double lambda, void* map_a, void* map_b, void* map_c, void* tmp, size_t* tmp_bytes,
                                  void* out_loss, void* stream) {
  int margin = 0;
  const int rc = ph_check(H, W, C, dtype, padding, "ms_photometric_fwd", &margin);
  if (rc) return rc;
  MS_CHECK_ARG(lambda >= 0.0 && lambda <= 1.0, "0 <= lambda <= 1 expected");
  const dim3 grid = dtype == MS_F32 ? ph_grid<float>(H, W, C) : ph_grid<double>(H, W, C);
  MS_CHECK_TMP(tmp, tmp_bytes, Carve::one((size_t)grid.x * grid.y * 2 * sizeof(double)));
  MS_CHECK_ARG(image && target && out_loss, "null pointer");
  MS_CHECK_ARG((map_a && map_b && map_c) || (!map_a && !map_b && !map_c), "the partial maps come as three or none");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MS_F32) ph_fwd<float>(image, target, H, W, C, margin, lambda, map_a, map_b, map_c, (double*)tmp, out_loss, s);
  else ph_fwd<double>(image, target, H, W, C, margin, lambda, map_a, map_b, map_c, (double*)tmp, out_loss, s);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_photometric_bwd(const void* image, const void* target, const void* map_a, const void* map_b,
                                  const void* map_c, const void* grad_out, int H, int W, int C, int dtype, int padding,
                                  double lambda, void* grad_image, void* stream) {
  int margin = 0;
  const int rc = ph_check(H, W, C, dtype, padding, "ms_photometric_bwd", &margin);
  if (rc) return rc;
  MS_CHECK_ARG(lambda >= 0.0 && lambda <= 1.0, "0 <= lambda <= 1 expected");
  MS_CHECK_ARG(image && target && map_a && map_b && map_c && grad_out && grad_image, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MS_F32) ph_bwd<float>(image, target, map_a, map_b, map_c, grad_out, H, W, C, margin, lambda, grad_image, s);
  else ph_bwd<double>(image, target, map_a, map_b, map_c, grad_out, H, W, C, margin, lambda, grad_image, s);
  MS_CHECK_LAUNCH();
  return 0;
}
