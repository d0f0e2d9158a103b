// bilagrid.hip — per-image appearance compensation of a 3-D gaussian-splatting trainer: the rendered (H, W, 3) image is
// sliced through a small learnable bilateral grid ("Bilateral guided radiance field processing") before the loss.
// The reference has no appearance model; the torch composition this replaces is a permute to a 5-D layout, a
// grid_sample gather of 8 corners x 12 planes per pixel, several (H, W, 12) intermediates and a backward that scatters
// into the grid with float atomics (not reproducible run to run).
//
// grid: (12, L, Gy, Gx), coefficient 4c + j = row c, column j of a 3 x 4 affine matrix.  For the pixel (y, x) of colour p:
//   gx = (x + 0.5) / W (Gx - 1)   gy = (y + 0.5) / H (Gy - 1)   gz = clamp(0.299 r + 0.587 g + 0.114 b, 0, 1) (L - 1)
//   A = trilinear interpolation of the 12 planes at (gz, gy, gx)     out = A[:, :3] p + A[:, 3]
// (grid_sample, bilinear, border, align_corners).  The cell of a coordinate is min(floor(coord), size - 2), 0 on an axis
// of size 1, which contributes its single plane with weight 1.  The clamp is written so that a NaN luminance lands in
// bin 0: it cannot address outside the grid.
//
// Forward and image gradient.  One lane per pixel, a workgroup (4 waves) owns 64 pixels x 16 rows.  The grid is
// plane-major, so the 8 corners x 12 coefficients of a pixel are 96 scattered 4-byte loads; but a tile touches few xy
// vertices when a cell is wider than the tile (2048^2 under 16 x 16: a cell is 136 pixels, a tile touches 4 to 6).  The
// workgroup stages the L x 12 coefficients of the vertices its tile touches in LDS, COEFFICIENT-INNERMOST, and a pixel
// reads each corner as 12 consecutive values (three ds_read_b128).  Where the footprint does not fit (a small image
// under a fine grid: the tile touches hundreds of vertices) the same code reads the corners from global memory, which
// for so small a grid is the L2.  The choice is per workgroup and uniform in it.
//
// Grid gradient, as a gather.  dL/dgrid[4c + j, z, yv, xv] = sum over pixels of w_z w_y w_x g_c p1_j.  A workgroup owns
// one xy vertex and one 64 x 64 chunk of that vertex's footprint |gx - xv| < 1, |gy - yv| < 1 (a conservative integer
// range; the weight zeroes what lies outside, and it is the forward's own cell arithmetic, so the two cannot disagree
// about a pixel).  A lane walks its 16 pixels and accumulates w g_c p1_j into ZB x 12 registers, one set per luminance
// bin, by evaluating the bin's weight: no data-dependent register index.  Then lane partials are promoted to double,
// summed over the wave by a butterfly and over the four waves in wave order, and the workgroup writes its (bins x 12)
// partial to tmp[vertex][chunk]; a second kernel adds a vertex's chunks in chunk order, in double, and writes the
// gradient in the grid's layout.  No atomics anywhere: the gradient is bit-reproducible; float32 is summed over runs of
// at most 16 pixels before the promotion, so the error does not grow with the pixel count.  Every element of the output
// is written (a vertex no pixel reaches gets exactly 0): the caller does not clear it.
#include <math.h>

#include "common.h"

namespace ms {

constexpr int BG_K = 12;                      // coefficients of one 3 x 4 matrix
constexpr int BG_TW = 64, BG_TH = 16;         // pixel tile of the forward and the image gradient
constexpr int BG_THREADS = 256;
constexpr int BG_WAVES = BG_THREADS / WAVE;
constexpr int BG_LDS = 4096;                  // staged coefficients per workgroup (16 KB float, 32 KB double): 42 vertices at L = 8
constexpr int BG_CW = 64, BG_CH = 64;         // chunk of a vertex's footprint in the grid gradient: 16 pixels per lane
constexpr int BG_MAX_L = 16, BG_MAX_G = 128;

template <typename T> struct BgDims {
  int H, W, L, Gy, Gx;
  T sx, sy;                                   // (Gx - 1) / W, (Gy - 1) / H
};

template <typename T> __device__ __forceinline__ T bg_coord(int i, T scale) { return (T(i) + T(0.5)) * scale; }

// cell of a finite coordinate >= 0 and the position inside it; size 1: cell 0 at position 0
template <typename T> __device__ __forceinline__ int bg_cell(T coord, int size, T& f) {
  int i = (int)coord;
  i = i < size - 2 ? i : size - 2;
  i = i > 0 ? i : 0;
  f = coord - T(i);
  return i;
}

// luminance -> (bin, position): NaN and everything <= 0 land at 0, +inf at 1
template <typename T> __device__ __forceinline__ int bg_bin(T lum, int L, T& f) {
  const T c = lum > T(0) ? (lum < T(1) ? lum : T(1)) : T(0);
  return bg_cell(c * T(L - 1), L, f);
}

template <typename T> __device__ __forceinline__ T bg_luminance(T r, T g, T b) {
  return T(0.299) * r + T(0.587) * g + T(0.114) * b;
}

// weight of vertex v for a coordinate in cell i at position f
template <typename T> __device__ __forceinline__ T bg_vertex_weight(int v, int i, T f) {
  return v == i ? T(1) - f : (v == i + 1 ? f : T(0));
}

// Pixels [lo, hi) of an axis of n pixels that can carry weight for vertex v of G: all with |coord - v| < 1, widened by a
// pixel (and by the float rounding of the coordinate, which passes half a pixel only beyond 2^20 pixels)
__host__ __device__ inline void bg_range(int v, int n, int G, int& lo, int& hi) {
  if (G == 1) { lo = 0; hi = n; return; }
  const int slack = 1 + (n >> 20);
  const int64_t a = (int64_t)(v > 0 ? v - 1 : 0) * n / (G - 1), b = (int64_t)(v + 1) * n / (G - 1);
  lo = a - slack > 0 ? (int)(a - slack) : 0;
  hi = b + 1 + slack < n ? (int)(b + 1 + slack) : n;
}

// ---- the eight corners of a pixel ------------------------------------------------------------------------------------
// at: first coefficient of the corner (iz, iy, ix); oz, ox, oy: distance to the second corner along each axis (0 on an
// axis of size 1: the same corner again, with weight 0); ks: distance between two coefficients of one corner
template <typename T> struct BgCorners {
  const T* at;
  int oz, ox, oy, ks;
};

template <typename T, bool STAGED>
__device__ __forceinline__ void bg_load(const T* p, int ks, T (&c)[BG_K]) {
  if (STAGED) {
    const T* q = (const T*)__builtin_assume_aligned(p, 16);
#pragma unroll
    for (int k = 0; k < BG_K; ++k) c[k] = q[k];
  } else {
#pragma unroll
    for (int k = 0; k < BG_K; ++k) c[k] = p[(int64_t)k * ks];
  }
}

// The vertices a tile of pixels touches: [x0v, x0v + nvx) x [y0v, y0v + nvy).  Staged into `s` as
// [vy][vx][z][12] when they fit (returns true; ends with a barrier), left alone otherwise.
template <typename T>
__device__ __forceinline__ bool bg_stage(T* s, const T* __restrict__ grid, const BgDims<T>& d, int col0, int row0,
                                         int& x0v, int& y0v, int& nvx) {
  const int col1 = (col0 + BG_TW < d.W ? col0 + BG_TW : d.W) - 1, row1 = (row0 + BG_TH < d.H ? row0 + BG_TH : d.H) - 1;
  T f;
  x0v = bg_cell(bg_coord<T>(col0, d.sx), d.Gx, f);
  y0v = bg_cell(bg_coord<T>(row0, d.sy), d.Gy, f);
  int x1v = bg_cell(bg_coord<T>(col1, d.sx), d.Gx, f) + 1, y1v = bg_cell(bg_coord<T>(row1, d.sy), d.Gy, f) + 1;
  x1v = x1v < d.Gx - 1 ? x1v : d.Gx - 1;
  y1v = y1v < d.Gy - 1 ? y1v : d.Gy - 1;
  nvx = x1v - x0v + 1;
  const int nvy = y1v - y0v + 1;
  const int count = nvx * nvy * d.L * BG_K;
  if (count > BG_LDS) return false;
  const int plane = d.Gy * d.Gx;
  for (int idx = threadIdx.x; idx < count; idx += BG_THREADS) {
    const int rest = idx / BG_K, k = idx - rest * BG_K;
    const int v = rest / d.L, z = rest - v * d.L;
    const int vy = v / nvx, vx = v - vy * nvx;
    s[idx] = grid[(int64_t)(k * d.L + z) * plane + (y0v + vy) * d.Gx + (x0v + vx)];
  }
  __syncthreads();
  return true;
}

template <typename T, bool STAGED>
__device__ __forceinline__ BgCorners<T> bg_corners(const T* s, const T* __restrict__ grid, const BgDims<T>& d, int x0v,
                                                   int y0v, int nvx, int ix, int iy, int iz) {
  BgCorners<T> c;
  if (STAGED) {
    c.at = s + (((iy - y0v) * nvx + (ix - x0v)) * d.L + iz) * BG_K;
    c.oz = d.L > 1 ? BG_K : 0;
    c.ox = d.Gx > 1 ? d.L * BG_K : 0;
    c.oy = d.Gy > 1 ? nvx * d.L * BG_K : 0;
    c.ks = 1;
  } else {
    const int plane = d.Gy * d.Gx;
    c.at = grid + ((int64_t)iz * plane + iy * d.Gx + ix);
    c.oz = d.L > 1 ? plane : 0;
    c.ox = d.Gx > 1 ? 1 : 0;
    c.oy = d.Gy > 1 ? d.Gx : 0;
    c.ks = d.L * plane;
  }
  return c;
}

// ---- forward -----------------------------------------------------------------------------------------------------------
template <typename T, bool STAGED>
__device__ __forceinline__ void bg_fwd_pixels(const T* s, const T* __restrict__ image, const T* __restrict__ grid,
                                              const BgDims<T>& d, int col0, int row0, int x0v, int y0v, int nvx,
                                              T* __restrict__ out) {
  const int col = col0 + lane_id(), wave = threadIdx.x / WAVE;
  if (col >= d.W) return;
  T fx;
  const int ix = bg_cell(bg_coord<T>(col, d.sx), d.Gx, fx);
#pragma unroll 1
  for (int i = 0; i < BG_TH / BG_WAVES; ++i) {
    const int row = row0 + wave + BG_WAVES * i;
    if (row >= d.H) break;
    const int64_t at = ((int64_t)row * d.W + col) * 3;
    const T r = image[at], g = image[at + 1], b = image[at + 2];
    T fy, fz;
    const int iy = bg_cell(bg_coord<T>(row, d.sy), d.Gy, fy);
    const int iz = bg_bin(bg_luminance(r, g, b), d.L, fz);
    const BgCorners<T> c = bg_corners<T, STAGED>(s, grid, d, x0v, y0v, nvx, ix, iy, iz);
    // interpolated as nested lerps u + f (v - u), z then x then y: where the corners agree (the identity grid) the
    // result is theirs exactly, and the identity grid returns the image bit for bit
    T a[BG_K], arow[BG_K];
#pragma unroll
    for (int corner = 0; corner < 4; ++corner) {
      const T* p = c.at + ((corner & 1) ? c.ox : 0) + ((corner & 2) ? c.oy : 0);
      T c0[BG_K], c1[BG_K];
      bg_load<T, STAGED>(p, c.ks, c0);
      bg_load<T, STAGED>(p + c.oz, c.ks, c1);
#pragma unroll
      for (int k = 0; k < BG_K; ++k) {
        const T v = c0[k] + fz * (c1[k] - c0[k]);
        if (corner == 0) a[k] = v;
        else if (corner == 1) a[k] += fx * (v - a[k]);
        else if (corner == 2) arow[k] = v;
        else a[k] += fy * (arow[k] + fx * (v - arow[k]) - a[k]);
      }
    }
    out[at] = a[0] * r + a[1] * g + a[2] * b + a[3];
    out[at + 1] = a[4] * r + a[5] * g + a[6] * b + a[7];
    out[at + 2] = a[8] * r + a[9] * g + a[10] * b + a[11];
  }
}

template <typename T>
__global__ void __launch_bounds__(BG_THREADS)
bilagrid_fwd_kernel(const T* __restrict__ image, const T* __restrict__ grid, BgDims<T> d, int tiles_x,
                    T* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) T s[BG_LDS];
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int col0 = tx * BG_TW, row0 = ty * BG_TH;
  int x0v, y0v, nvx;
  if (bg_stage(s, grid, d, col0, row0, x0v, y0v, nvx)) bg_fwd_pixels<T, true>(s, image, grid, d, col0, row0, x0v, y0v, nvx, out);
  else bg_fwd_pixels<T, false>(s, image, grid, d, col0, row0, x0v, y0v, nvx, out);
}

// ---- image gradient ----------------------------------------------------------------------------------------------------
// dL/dp_j = sum_c g_c A[c][j] + [0 < lum < 1] (L - 1) (sum_k g_c p1_j dA/dgz[k]) lumcoef_j, dA/dgz = the xy-interpolated
// difference of the cell's two luminance planes
template <typename T, bool STAGED>
__device__ __forceinline__ void bg_image_grad_pixels(const T* s, const T* __restrict__ image, const T* __restrict__ grid,
                                                     const T* __restrict__ grad_out, const BgDims<T>& d, int col0,
                                                     int row0, int x0v, int y0v, int nvx, T* __restrict__ grad_image) {
  const int col = col0 + lane_id(), wave = threadIdx.x / WAVE;
  if (col >= d.W) return;
  T fx;
  const int ix = bg_cell(bg_coord<T>(col, d.sx), d.Gx, fx);
#pragma unroll 1
  for (int i = 0; i < BG_TH / BG_WAVES; ++i) {
    const int row = row0 + wave + BG_WAVES * i;
    if (row >= d.H) break;
    const int64_t at = ((int64_t)row * d.W + col) * 3;
    const T p1[4] = {image[at], image[at + 1], image[at + 2], T(1)};
    const T go[3] = {grad_out[at], grad_out[at + 1], grad_out[at + 2]};
    T fy, fz;
    const int iy = bg_cell(bg_coord<T>(row, d.sy), d.Gy, fy);
    const T lum = bg_luminance(p1[0], p1[1], p1[2]);
    const int iz = bg_bin(lum, d.L, fz);
    const BgCorners<T> c = bg_corners<T, STAGED>(s, grid, d, x0v, y0v, nvx, ix, iy, iz);
    // per xy corner: v[j] = sum_c g_c A[c][j] at gz (j < 3) and v[3] = sum_k g_c p1_j (plane iz + 1 - plane iz)[k];
    // the four corners are then interpolated as the forward does, x then y
    T q[4], qrow[4];
#pragma unroll
    for (int corner = 0; corner < 4; ++corner) {
      const T* p = c.at + ((corner & 1) ? c.ox : 0) + ((corner & 2) ? c.oy : 0);
      T c0[BG_K], c1[BG_K];
      bg_load<T, STAGED>(p, c.ks, c0);
      bg_load<T, STAGED>(p + c.oz, c.ks, c1);
      T v[4] = {T(0), T(0), T(0), T(0)};
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = 4 * ch + j;
          const T dz = c1[k] - c0[k];
          if (j < 3) v[j] += go[ch] * (c0[k] + fz * dz);
          v[3] += (go[ch] * p1[j]) * dz;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (corner == 0) q[j] = v[j];
        else if (corner == 1) q[j] += fx * (v[j] - q[j]);
        else if (corner == 2) qrow[j] = v[j];
        else q[j] += fy * (qrow[j] + fx * (v[j] - qrow[j]) - q[j]);
      }
    }
    const T guide = (lum > T(0) && lum < T(1)) ? T(d.L - 1) * q[3] : T(0);
    grad_image[at] = q[0] + guide * T(0.299);
    grad_image[at + 1] = q[1] + guide * T(0.587);
    grad_image[at + 2] = q[2] + guide * T(0.114);
  }
}

template <typename T>
__global__ void __launch_bounds__(BG_THREADS)
bilagrid_image_grad_kernel(const T* __restrict__ image, const T* __restrict__ grid, const T* __restrict__ grad_out,
                           BgDims<T> d, int tiles_x, T* __restrict__ grad_image) {
  __shared__ __attribute__((aligned(16))) T s[BG_LDS];
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int col0 = tx * BG_TW, row0 = ty * BG_TH;
  int x0v, y0v, nvx;
  if (bg_stage(s, grid, d, col0, row0, x0v, y0v, nvx))
    bg_image_grad_pixels<T, true>(s, image, grid, grad_out, d, col0, row0, x0v, y0v, nvx, grad_image);
  else
    bg_image_grad_pixels<T, false>(s, image, grid, grad_out, d, col0, row0, x0v, y0v, nvx, grad_image);
}

// ---- grid gradient -----------------------------------------------------------------------------------------------------
// blockIdx = (chunk of the footprint, xy vertex, group of ZB luminance bins); tmp: [vertex][chunk][L][12] doubles
template <typename T, int ZB>
__global__ void __launch_bounds__(BG_THREADS)
bilagrid_grid_grad_kernel(const T* __restrict__ image, const T* __restrict__ grad_out, BgDims<T> d, int chunks_x,
                          double* __restrict__ tmp) {
  __shared__ double red[BG_WAVES][ZB * BG_K];
  const int chunk = blockIdx.x, vertex = blockIdx.y, z0 = blockIdx.z * ZB;
  const int yv = vertex / d.Gx, xv = vertex - yv * d.Gx;
  const int cy = chunk / chunks_x, cx = chunk - cy * chunks_x;
  const int lane = lane_id(), wave = threadIdx.x / WAVE;
  int x_lo, x_hi, y_lo, y_hi;
  bg_range(xv, d.W, d.Gx, x_lo, x_hi);
  bg_range(yv, d.H, d.Gy, y_lo, y_hi);
  const int col = x_lo + cx * BG_CW + lane;

  T acc[ZB][BG_K];
#pragma unroll
  for (int z = 0; z < ZB; ++z)
#pragma unroll
    for (int k = 0; k < BG_K; ++k) acc[z][k] = T(0);

  T wx = T(0);
  if (col < x_hi) {
    T fx;
    const int ix = bg_cell(bg_coord<T>(col, d.sx), d.Gx, fx);
    wx = bg_vertex_weight(xv, ix, fx);
  }
  if (wx != T(0)) {
#pragma unroll 1
    for (int i = 0; i < BG_CH / BG_WAVES; ++i) {
      const int row = y_lo + cy * BG_CH + wave + BG_WAVES * i;
      if (row >= y_hi) break;
      T fy, fz;
      const int iy = bg_cell(bg_coord<T>(row, d.sy), d.Gy, fy);
      const T w = wx * bg_vertex_weight(yv, iy, fy);
      if (w == T(0)) continue;
      const int64_t at = ((int64_t)row * d.W + col) * 3;
      const T p1[4] = {image[at], image[at + 1], image[at + 2], T(1)};
      const int iz = bg_bin(bg_luminance(p1[0], p1[1], p1[2]), d.L, fz);
      T gp[BG_K];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const T g = w * grad_out[at + ch];
#pragma unroll
        for (int j = 0; j < 4; ++j) gp[4 * ch + j] = g * p1[j];
      }
#pragma unroll
      for (int z = 0; z < ZB; ++z) {
        const T wz = bg_vertex_weight(z0 + z, iz, fz);
#pragma unroll
        for (int k = 0; k < BG_K; ++k) acc[z][k] += wz * gp[k];
      }
    }
  }

  // lane partials -> double -> wave butterfly -> the four waves in wave order
#pragma unroll
  for (int z = 0; z < ZB; ++z) {
#pragma unroll
    for (int k = 0; k < BG_K; ++k) {
      const double t = wave_sum_to_lane63((double)acc[z][k]);
      if (lane == WAVE - 1) red[wave][z * BG_K + k] = t;
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < ZB * BG_K && z0 + t / BG_K < d.L) {
    double sum = red[0][t];
    for (int w = 1; w < BG_WAVES; ++w) sum += red[w][t];
    tmp[((int64_t)vertex * gridDim.x + chunk) * (d.L * BG_K) + z0 * BG_K + t] = sum;
  }
}

// one lane per element of the gradient: its vertex's chunks in chunk order, in double, written in the grid's layout
template <typename T>
__global__ void __launch_bounds__(BG_THREADS)
bilagrid_grid_finalize_kernel(const double* __restrict__ tmp, int chunks, int L, int plane, T* __restrict__ grad_grid) {
  const int o = blockIdx.x * BG_THREADS + threadIdx.x;
  const int row = L * BG_K;
  if (o >= plane * row) return;
  const int vertex = o / row, zk = o - vertex * row;
  const int z = zk / BG_K, k = zk - z * BG_K;
  const double* p = tmp + (int64_t)vertex * chunks * row + zk;
  double sum = 0.0;
  for (int c = 0; c < chunks; ++c) sum += p[(int64_t)c * row];
  grad_grid[(int64_t)(k * L + z) * plane + vertex] = (T)sum;
}

// ---- host --------------------------------------------------------------------------------------------------------------
static int bg_extent(int n, int G) {          // widest footprint of a vertex along an axis
  int widest = 0;
  for (int v = 0; v < G; ++v) {
    int lo, hi;
    bg_range(v, n, G, lo, hi);
    widest = hi - lo > widest ? hi - lo : widest;
  }
  return widest;
}

struct BgChunks { int64_t x, y; };

static BgChunks bg_chunks(int H, int W, int Gy, int Gx) {
  return BgChunks{div_up(bg_extent(W, Gx), BG_CW), div_up(bg_extent(H, Gy), BG_CH)};
}

template <typename T> static BgDims<T> bg_dims(int H, int W, int L, int Gy, int Gx) {
  return BgDims<T>{H, W, L, Gy, Gx, (T)((double)(Gx - 1) / W), (T)((double)(Gy - 1) / H)};
}

template <typename T>
static void bg_fwd(const void* image, const void* grid, int H, int W, int L, int Gy, int Gx, void* out, hipStream_t s) {
  const int64_t tiles_x = div_up(W, BG_TW), tiles_y = div_up(H, BG_TH);
  bilagrid_fwd_kernel<T><<<dim3((unsigned)(tiles_x * tiles_y)), dim3(BG_THREADS), 0, s>>>(
      (const T*)image, (const T*)grid, bg_dims<T>(H, W, L, Gy, Gx), (int)tiles_x, (T*)out);
}

template <typename T>
static void bg_bwd(const void* image, const void* grid, const void* grad_out, int H, int W, int L, int Gy, int Gx,
                   void* grad_image, void* grad_grid, double* tmp, hipStream_t s) {
  const BgDims<T> d = bg_dims<T>(H, W, L, Gy, Gx);
  if (grad_image) {
    const int64_t tiles_x = div_up(W, BG_TW), tiles_y = div_up(H, BG_TH);
    bilagrid_image_grad_kernel<T><<<dim3((unsigned)(tiles_x * tiles_y)), dim3(BG_THREADS), 0, s>>>(
        (const T*)image, (const T*)grid, (const T*)grad_out, d, (int)tiles_x, (T*)grad_image);
  }
  if (grad_grid) {
    const BgChunks c = bg_chunks(H, W, Gy, Gx);
    const int chunks = (int)(c.x * c.y), plane = Gy * Gx;
    if (L <= 2)
      bilagrid_grid_grad_kernel<T, 2><<<dim3(chunks, plane, 1), dim3(BG_THREADS), 0, s>>>(
          (const T*)image, (const T*)grad_out, d, (int)c.x, tmp);
    else
      bilagrid_grid_grad_kernel<T, 8><<<dim3(chunks, plane, (unsigned)div_up(L, 8)), dim3(BG_THREADS), 0, s>>>(
          (const T*)image, (const T*)grad_out, d, (int)c.x, tmp);
    bilagrid_grid_finalize_kernel<T><<<dim3((unsigned)div_up((int64_t)plane * L * BG_K, BG_THREADS)), dim3(BG_THREADS), 0, s>>>(
        tmp, chunks, L, plane, (T*)grad_grid);
  }
}

}  // namespace ms

using namespace ms;

static int bg_check(int H, int W, int L, int Gy, int Gx, int dtype, const char* who) {
  if (H <= 0 || W <= 0) { set_error("%s: H, W > 0 expected (got %d x %d)", who, H, W); return MS_ERR_BAD_ARG; }
  if (L <= 0 || Gy <= 0 || Gx <= 0) {
    set_error("%s: L, Gy, Gx > 0 expected (got %d, %d, %d)", who, L, Gy, Gx);
    return MS_ERR_BAD_ARG;
  }
  if (L > BG_MAX_L || Gy > BG_MAX_G || Gx > BG_MAX_G) {
    set_error("%s: grid (L %d, Gy %d, Gx %d) beyond L <= %d, Gy, Gx <= %d", who, L, Gy, Gx, BG_MAX_L, BG_MAX_G);
    return MS_ERR_UNSUPPORTED;
  }
  if ((int64_t)H * W * 3 > INT32_MAX) { set_error("%s: image too large (%d x %d x 3)", who, H, W); return MS_ERR_UNSUPPORTED; }
  if (dtype != MS_F32 && dtype != MS_F64) { set_error("%s: unknown dtype %d", who, dtype); return MS_ERR_UNSUPPORTED; }
  return 0;
}

extern "C" int ms_bilagrid_fwd(const void* image, const void* grid, int H, int W, int L, int Gy, int Gx, int dtype,
                               void* out, void* stream) {
  const int rc = bg_check(H, W, L, Gy, Gx, dtype, "ms_bilagrid_fwd");
  if (rc) return rc;
  MS_CHECK_ARG(image && grid && out, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MS_F32) bg_fwd<float>(image, grid, H, W, L, Gy, Gx, out, s);
  else bg_fwd<double>(image, grid, H, W, L, Gy, Gx, out, s);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_bilagrid_bwd(const void* image, const void* grid, const void* grad_out, int H, int W, int L, int Gy,
                               int Gx, int dtype, void* grad_image, void* grad_grid, void* tmp, size_t* tmp_bytes,
                               void* stream) {
  const int rc = bg_check(H, W, L, Gy, Gx, dtype, "ms_bilagrid_bwd");
  if (rc) return rc;
  const BgChunks c = bg_chunks(H, W, Gy, Gx);
  MS_CHECK_TMP(tmp, tmp_bytes, Carve::one((size_t)(c.x * c.y) * Gy * Gx * L * BG_K * sizeof(double)));
  MS_CHECK_ARG(image && grid && grad_out, "null pointer");
  MS_CHECK_ARG(grad_image || grad_grid, "grad_image and grad_grid are both null: nothing to compute");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == MS_F32) bg_bwd<float>(image, grid, grad_out, H, W, L, Gy, Gx, grad_image, grad_grid, (double*)tmp, s);
  else bg_bwd<double>(image, grid, grad_out, H, W, L, Gy, Gx, grad_image, grad_grid, (double*)tmp, s);
  MS_CHECK_LAUNCH();
  return 0;
}
