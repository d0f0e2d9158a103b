// tsdf.hip — fuse depth frames into a truncated signed distance volume and triangulate it (no reference counterpart:
// an addition; the step 2DGS, GOF and PGSR take from rendered depth to a mesh).
//
// The volume is (nz, ny, nx) float32, x fastest, samples on grid vertices p(i, j, k) = origin + voxel (i, j, k).
// Kernels of this file = 3 (tests/test_tsdf_budgets.py holds the count, 0 bytes of scratch and the registers):
//
// tsdf_integrate_kernel   ONE launch for all C frames of a call.  A lane owns TSDF_RUN = 4 consecutive samples of the
//   linear order (a run along x; with nx % 4 != 0 a run may wrap into the next row, every sample derives its own
//   (i, j, k)), so tsdf and weight move as one 16-byte access each and colour as three.  Its values stay in registers over
//   the whole camera loop: a call with C frames reads and writes the volume once.  Per sample and camera, in camera
//   order, the rule of include/mi355_splat.h, no FMA contraction (the comparisons are shared with the float32 torch
//   composition and the oracle).
//   Culling: every wave of a workgroup tests the box of its own 256 samples against each camera's clip range and the
//   four side planes of its frustum — lane b of the wave takes camera base + b, TSDF_CHUNK = 64 cameras per ballot, so
//   the test costs one camera per lane, not one per lane and camera.  The test is conservative (a relative slack of
//   1e-4 on the magnitudes that enter it, a hundred float32 roundings; a NaN keeps the camera), and a culled camera
//   could not have passed the per-sample tests, so it changes no result.  The ballot is wave-uniform: the loop over the
//   surviving cameras reads their rows through the scalar cache, as camera_coverage.hip does.  A wave no camera
//   survives for touches the volume neither for read nor for write; a lane none of whose samples was updated does not
//   store; a skipped sample of a lane that stores gets the bits it was loaded with.
//   No atomics.  The chunks do not show: a sample sees the cameras in ascending order whatever the ballots were.
//
// tsdf_classify_kernel    one lane per grid vertex o: the 7-bit mask of the mesh vertices on the edges o owns
//   (o -> o + d, d = 100 010 001 110 101 011 111 in x y z bits, both ends valid and of different sign) and the number
//   of triangles of the cell whose lower corner is o (0..12), as word = mask | triangles << 8, and the two counts as
//   the inputs of the two scans.
// tsdf_emit_kernel        one lane per grid vertex with word != 0: its vertices at vscan[o] + rank, its cell's
//   triangles at tscan[o] + running index; a triangle finds a vertex as vscan[owner] + popcount(mask[owner] & ((1 << e) - 1)).
//
// Marching tetrahedra on the Kuhn split: tetrahedron tau = 0..5 is the corner path 0 -> 1 << a0 -> ... -> 7 of the
// axis permutation (a0, a1, a2) in lexicographic order.  The 16 sign cases of a tetrahedron are generated at compile
// time (tet_case below): with the inside corners listed first,
//   one corner a apart from b < c < d     triangle (ab, ac, ad)
//   inside a < b, outside c < d           triangles (ac, bd, bc) and (ac, ad, bd)
// as written when (a, b, c, d) is an even permutation of the path and a is inside, the last two swapped otherwise, and
// swapped once more in a tetrahedron of an odd axis permutation: (b - a) x (c - a) points to the positive side.
#pragma clang fp contract(off)
#include "common.h"

namespace ms {

constexpr int TSDF_RUN = MS_TSDF_RUN;
constexpr int TSDF_CHUNK = MS_TSDF_CAMERA_CHUNK;
constexpr int TSDF_CAMERA = MS_COVERAGE_CAMERA_VALUES;
static_assert(TSDF_RUN == 4 && TSDF_CHUNK == 64 && TSDF_CAMERA == 20, "16-byte runs, one ballot per chunk, 20-value camera rows");

struct TsdfGrid {
  int nx, ny, nz;
  float ox, oy, oz, voxel;
};

__device__ __forceinline__ void tsdf_split(int linear, const TsdfGrid& g, int& i, int& j, int& k) {
  const int row = linear / g.nx;
  i = linear - row * g.nx;
  k = row / g.ny;
  j = row - k * g.ny;
}

// May a sample of the box [lo, hi] (grid indices, inclusive) pass camera `row`'s depth and image tests?  Conservative.
__device__ __forceinline__ bool tsdf_box_may_be_seen(const float* __restrict__ row, const TsdfGrid& g, const int (&lo)[3],
                                                     const int (&hi)[3], float width, float height) {
  const float origin[3] = {g.ox, g.oy, g.oz};
  float centre[3], half[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    centre[a] = origin[a] + g.voxel * (0.5f * (float)(lo[a] + hi[a]));
    half[a] = fabsf(g.voxel) * (0.5f * (float)(hi[a] - lo[a]));
  }
  float z = row[11], z_magnitude = fabsf(row[11]), z_radius = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    z += row[8 + a] * centre[a];
    z_magnitude += fabsf(row[8 + a]) * (fabsf(centre[a]) + half[a]);
    z_radius += fabsf(row[8 + a]) * half[a];
  }
  const float near_plane = row[16], far_plane = row[17];
  const float z_slack = 1e-4f * z_magnitude;
  if (z + z_radius + z_slack < near_plane) return false;
  if (z - z_radius - z_slack > far_plane) return false;
  if (!(near_plane > 0.f)) return true;                 // the side planes below assume z > 0 for every sample that passes
  // u = f x / z + c in [0, size)  <=>  f x + c z >= 0  and  f x + (c - size) z < 0   (z > 0): linear in the sample
#pragma unroll
  for (int axis = 0; axis < 2; ++axis) {
    const float f = row[12 + axis], c = row[14 + axis], size = axis == 0 ? width : height;
    float mag = fabsf(row[axis * 4 + 3]);
#pragma unroll
    for (int a = 0; a < 3; ++a) mag += fabsf(row[axis * 4 + a]) * (fabsf(centre[a]) + half[a]);
    const float slack = 1e-4f * (fabsf(f) * mag + (fabsf(c) + size) * z_magnitude);
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const float cz = side == 0 ? c : c - size;
      float at_centre = f * row[axis * 4 + 3] + cz * row[11];
      float radius = 0.f;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float coefficient = f * row[axis * 4 + a] + cz * row[8 + a];
        at_centre += coefficient * centre[a];
        radius += fabsf(coefficient) * half[a];
      }
      if (side == 0 ? at_centre + radius + slack < 0.f : at_centre - radius - slack > 0.f) return false;
    }
  }
  return true;
}

__global__ void __launch_bounds__(256)
tsdf_integrate_kernel(float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ colour, TsdfGrid g, int n,
                      float truncation, float max_weight, const float* __restrict__ depth,
                      const float* __restrict__ pixel_weight, const float* __restrict__ image,
                      const float* __restrict__ cameras, int num_cameras, int width, int height) {
  const int run = blockIdx.x * 256 + threadIdx.x;
  const int lane = lane_id();
  const int first = run * TSDF_RUN;
  const int wave_first = __builtin_amdgcn_readfirstlane(first);
  if (wave_first >= n) return;
  const int wave_last = (wave_first + WAVE * TSDF_RUN < n ? wave_first + WAVE * TSDF_RUN : n) - 1;

  int lo[3], hi[3];
  {
    int a[3], b[3];
    tsdf_split(wave_first, g, a[0], a[1], a[2]);
    tsdf_split(wave_last, g, b[0], b[1], b[2]);
    const bool same_slice = a[2] == b[2], same_row = same_slice && a[1] == b[1];
    lo[2] = a[2]; hi[2] = b[2];
    lo[1] = same_slice ? a[1] : 0; hi[1] = same_slice ? b[1] : g.ny - 1;
    lo[0] = same_row ? a[0] : 0; hi[0] = same_row ? b[0] : g.nx - 1;
  }

  const int mine = first >= n ? 0 : (n - first < TSDF_RUN ? n - first : TSDF_RUN);
  float px[TSDF_RUN], py[TSDF_RUN], pz[TSDF_RUN];
  {
    int i = 0, j = 0, k = 0;
    if (mine > 0) tsdf_split(first, g, i, j, k);
#pragma unroll
    for (int s = 0; s < TSDF_RUN; ++s) {
      px[s] = g.ox + g.voxel * (float)i;                // from (i, j, k), never stepped
      py[s] = g.oy + g.voxel * (float)j;
      pz[s] = g.oz + g.voxel * (float)k;
      if (++i == g.nx) { i = 0; if (++j == g.ny) { j = 0; ++k; } }
    }
  }

  const float fwidth = (float)width, fheight = (float)height;
  float t[TSDF_RUN], w[TSDF_RUN], col[TSDF_RUN * 3];
  bool loaded = false, touched = false;

#pragma unroll 1
  for (int base = 0; base < num_cameras; base += TSDF_CHUNK) {
    bool keep = false;
    if (base + lane < num_cameras)
      keep = tsdf_box_may_be_seen(cameras + (size_t)(base + lane) * TSDF_CAMERA, g, lo, hi, fwidth, fheight);
    unsigned long long live = __ballot(keep);
    if (live == 0) continue;
    if (!loaded) {
      loaded = true;
      if (mine == TSDF_RUN) {
        const float4 tv = *reinterpret_cast<const float4*>(tsdf + first);
        const float4 wv = *reinterpret_cast<const float4*>(weight + first);
        t[0] = tv.x; t[1] = tv.y; t[2] = tv.z; t[3] = tv.w;
        w[0] = wv.x; w[1] = wv.y; w[2] = wv.z; w[3] = wv.w;
        if (colour) {
#pragma unroll
          for (int v = 0; v < 3; ++v) {
            const float4 cv = *reinterpret_cast<const float4*>(colour + (size_t)first * 3 + v * 4);
            col[v * 4 + 0] = cv.x; col[v * 4 + 1] = cv.y; col[v * 4 + 2] = cv.z; col[v * 4 + 3] = cv.w;
          }
        }
      } else {
#pragma unroll
        for (int s = 0; s < TSDF_RUN; ++s) {
          const bool in = s < mine;
          t[s] = in ? tsdf[first + s] : 1.f;
          w[s] = in ? weight[first + s] : 0.f;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) col[s * 3 + ch] = (in && colour) ? colour[(size_t)(first + s) * 3 + ch] : 0.f;
        }
      }
    }
#pragma unroll 1
    while (live) {
      const int b = __builtin_ctzll(live);
      live &= live - 1;
      const int c = base + b;                                           // wave-uniform
      const float* __restrict__ row = cameras + (size_t)c * TSDF_CAMERA;
      const float near_plane = row[16], far_plane = row[17];
      const float fx = row[12], fy = row[13], cx = row[14], cy = row[15];
#pragma unroll
      for (int s = 0; s < TSDF_RUN; ++s) {
        if (s >= mine) continue;
        const float z = row[8] * px[s] + row[9] * py[s] + row[10] * pz[s] + row[11];
        if (!(z >= near_plane && z <= far_plane)) continue;
        const float x = row[0] * px[s] + row[1] * py[s] + row[2] * pz[s] + row[3];
        const float y = row[4] * px[s] + row[5] * py[s] + row[6] * pz[s] + row[7];
        const float u = fx * x / z + cx, v = fy * y / z + cy;
        if (!(u >= 0.f && u < fwidth && v >= 0.f && v < fheight)) continue;      // floor(u) in [0, W); a NaN skips
        const int ix = (int)u, iy = (int)v;                                          // truncation = floor for u >= 0
        const size_t pixel = ((size_t)c * height + iy) * width + ix;
        const float d = depth[pixel];
        if (!(d > 0.f && d < __builtin_huge_valf())) continue;
        const float pw = pixel_weight ? pixel_weight[pixel] : 1.f;
        if (!(pw > 0.f)) continue;
        const float sd = d - z;
        if (sd < -truncation) continue;
        const float tv = fminf(1.f, sd / truncation);
        const float sum = w[s] + pw;
        t[s] = (w[s] * t[s] + pw * tv) / sum;
        if (colour) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) col[s * 3 + ch] = (w[s] * col[s * 3 + ch] + pw * image[pixel * 3 + ch]) / sum;
        }
        w[s] = fminf(sum, max_weight);
        touched = true;
      }
    }
  }

  if (!touched) return;
  if (mine == TSDF_RUN) {
    *reinterpret_cast<float4*>(tsdf + first) = make_float4(t[0], t[1], t[2], t[3]);
    *reinterpret_cast<float4*>(weight + first) = make_float4(w[0], w[1], w[2], w[3]);
    if (colour) {
#pragma unroll
      for (int v = 0; v < 3; ++v)
        *reinterpret_cast<float4*>(colour + (size_t)first * 3 + v * 4) =
            make_float4(col[v * 4 + 0], col[v * 4 + 1], col[v * 4 + 2], col[v * 4 + 3]);
    }
  } else {
#pragma unroll
    for (int s = 0; s < TSDF_RUN; ++s) {
      if (s >= mine) continue;
      tsdf[first + s] = t[s];
      weight[first + s] = w[s];
      if (colour) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) colour[(size_t)(first + s) * 3 + ch] = col[s * 3 + ch];
      }
    }
  }
}

// ---- marching tetrahedra -----------------------------------------------------------------------------------------------

// edge type of a direction code (x = 1, y = 2, z = 4): the order 100 010 001 110 101 011 111 of the contract
__device__ __forceinline__ constexpr int tsdf_edge_type(int code) {
  return code == 1 ? 0 : code == 2 ? 1 : code == 4 ? 2 : code == 3 ? 3 : code == 5 ? 4 : code == 6 ? 5 : 6;
}
__device__ __forceinline__ constexpr int tsdf_direction_of_type(int type) {
  return type == 0 ? 1 : type == 1 ? 2 : type == 2 ? 4 : type == 3 ? 3 : type == 4 ? 5 : type == 5 ? 6 : 7;
}

// corner `v` (0..3) of tetrahedron `tau` (0..5) as a corner code of the cell; an odd axis permutation mirrors it
__device__ __forceinline__ constexpr int tsdf_tet_corner(int tau, int v) {
  const int a0 = tau >> 1;
  const int a1 = (tau & 1) == 0 ? (a0 == 0 ? 1 : 0) : (a0 == 2 ? 1 : 2);      // lexicographic: the smaller free axis first
  return v == 0 ? 0 : v == 1 ? 1 << a0 : v == 2 ? (1 << a0) | (1 << a1) : 7;
}
__device__ __forceinline__ constexpr bool tsdf_tet_mirrored(int tau) { return tau == 1 || tau == 2 || tau == 5; }

struct TetCases { uint32_t word[16]; };

// case word: triangles (0..2) | 3 x 4 bits per triangle, each an edge (low path corner << 2 | high path corner)
constexpr uint32_t tet_edge(int a, int b) { return a < b ? (uint32_t)(a << 2 | b) : (uint32_t)(b << 2 | a); }
constexpr uint32_t tet_triangle(uint32_t e0, uint32_t e1, uint32_t e2, bool flip) {
  return flip ? e0 | e2 << 4 | e1 << 8 : e0 | e1 << 4 | e2 << 8;
}
constexpr uint32_t tet_case(int inside_bits) {
  int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, nin = 0, nout = 0;
  for (int v = 0; v < 4; ++v) {
    if (inside_bits >> v & 1) in[nin++] = v; else out[nout++] = v;
  }
  if (nin == 0 || nin == 4) return 0;
  if (nin == 2) {
    const int a = in[0], b = in[1], c = out[0], d = out[1];
    const int order[4] = {a, b, c, d};
    int inversions = 0;
    for (int p = 0; p < 4; ++p)
      for (int q = p + 1; q < 4; ++q) inversions += order[p] > order[q];
    const bool flip = inversions & 1;
    return 2u | tet_triangle(tet_edge(a, c), tet_edge(b, d), tet_edge(b, c), flip) << 2
              | tet_triangle(tet_edge(a, c), tet_edge(a, d), tet_edge(b, d), flip) << 14;
  }
  const int a = nin == 1 ? in[0] : out[0];
  const int* rest = nin == 1 ? out : in;
  const bool flip = ((a & 1) != 0) != (nin == 3);       // (a, b, c, d) with b < c < d has a inversions
  return 1u | tet_triangle(tet_edge(a, rest[0]), tet_edge(a, rest[1]), tet_edge(a, rest[2]), flip) << 2;
}
constexpr TetCases make_tet_cases() {
  TetCases cases{};
  for (int m = 0; m < 16; ++m) cases.word[m] = tet_case(m);
  return cases;
}
__constant__ TetCases TET_CASES = make_tet_cases();

// valid and inside bits of the 8 corners of the cell at o (bit = corner code); corners outside the grid are invalid
__device__ __forceinline__ void tsdf_corners(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                             const TsdfGrid& g, int o, int i, int j, int k, float min_weight,
                                             uint32_t& valid, uint32_t& inside, float (&value)[8]) {
  valid = 0; inside = 0;
#pragma unroll
  for (int code = 0; code < 8; ++code) {
    const int dx = code & 1, dy = code >> 1 & 1, dz = code >> 2;
    value[code] = 1.f;
    if (i + dx < g.nx && j + dy < g.ny && k + dz < g.nz) {
      const int at = o + dx + (dy + dz * g.ny) * g.nx;
      const float wv = weight[at];
      value[code] = tsdf[at];
      if (wv > 0.f && wv >= min_weight) valid |= 1u << code;
      if (value[code] < 0.f) inside |= 1u << code;
    }
  }
}

__device__ __forceinline__ uint32_t tsdf_tet_case_bits(int tau, uint32_t valid, uint32_t inside, bool& all_valid) {
  uint32_t bits = 0;
  all_valid = true;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int code = tsdf_tet_corner(tau, v);
    all_valid = all_valid && (valid >> code & 1);
    bits |= (inside >> code & 1) << v;
  }
  return bits;
}

__global__ void __launch_bounds__(256)
tsdf_classify_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight, TsdfGrid g, int n, float min_weight,
                     int32_t* __restrict__ word, int32_t* __restrict__ vertex_count, int32_t* __restrict__ triangle_count) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= n) return;
  int i, j, k;
  tsdf_split(o, g, i, j, k);
  uint32_t valid, inside;
  float value[8];
  tsdf_corners(tsdf, weight, g, o, i, j, k, min_weight, valid, inside, value);
  uint32_t mask = 0;
  if (valid & 1u) {
#pragma unroll
    for (int code = 1; code < 8; ++code)
      if ((valid >> code & 1) && ((inside >> code & 1) != (inside & 1u))) mask |= 1u << tsdf_edge_type(code);
  }
  int triangles = 0;
  if ((valid & 0x81u) == 0x81u && inside != 0 && inside != 0xffu) {     // every tetrahedron holds corners 0 and 7
#pragma unroll
    for (int tau = 0; tau < 6; ++tau) {
      bool all_valid;
      const uint32_t bits = tsdf_tet_case_bits(tau, valid, inside, all_valid);
      if (all_valid) triangles += (int)(TET_CASES.word[bits] & 3u);
    }
  }
  word[o] = (int32_t)(mask | (uint32_t)triangles << 8);
  vertex_count[o] = __popc(mask);
  triangle_count[o] = triangles;
}

__global__ void __launch_bounds__(256)
tsdf_emit_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight, const float* __restrict__ colour,
                 TsdfGrid g, int n, float min_weight, const int32_t* __restrict__ word,
                 const int32_t* __restrict__ vertex_scan, const int32_t* __restrict__ triangle_scan,
                 float* __restrict__ out_vertices, int32_t* __restrict__ out_faces, float* __restrict__ out_colours) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= n) return;
  const uint32_t mine = (uint32_t)word[o];
  if (mine == 0) return;
  int i, j, k;
  tsdf_split(o, g, i, j, k);
  uint32_t valid, inside;
  float value[8];
  tsdf_corners(tsdf, weight, g, o, i, j, k, min_weight, valid, inside, value);

  const uint32_t mask = mine & 0x7fu;
  if (mask) {
    const float p[3] = {g.ox + g.voxel * (float)i, g.oy + g.voxel * (float)j, g.oz + g.voxel * (float)k};
    size_t at = (size_t)vertex_scan[o];
#pragma unroll
    for (int type = 0; type < 7; ++type) {
      if (!(mask >> type & 1)) continue;
      const int code = tsdf_direction_of_type(type);
      const int dx = code & 1, dy = code >> 1 & 1, dz = code >> 2;
      const float lambda = value[0] / (value[0] - value[code]);
      const float q[3] = {g.ox + g.voxel * (float)(i + dx), g.oy + g.voxel * (float)(j + dy), g.oz + g.voxel * (float)(k + dz)};
#pragma unroll
      for (int a = 0; a < 3; ++a) out_vertices[at * 3 + a] = p[a] + lambda * (q[a] - p[a]);
      if (out_colours) {
        const size_t far_end = (size_t)(o + dx + (dy + dz * g.ny) * g.nx);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float c0 = colour[(size_t)o * 3 + ch], c1 = colour[far_end * 3 + ch];
          out_colours[at * 3 + ch] = c0 + lambda * (c1 - c0);
        }
      }
      ++at;
    }
  }

  if ((mine >> 8) == 0) return;
  size_t face = (size_t)triangle_scan[o];
#pragma unroll
  for (int tau = 0; tau < 6; ++tau) {
    bool all_valid;
    const uint32_t bits = tsdf_tet_case_bits(tau, valid, inside, all_valid);
    if (!all_valid) continue;
    uint32_t entry = TET_CASES.word[bits];
    const int triangles = (int)(entry & 3u);
    entry >>= 2;
    for (int r = 0; r < triangles; ++r) {
      int index[3];
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        const uint32_t edge = entry & 15u;
        entry >>= 4;
        int low = 0, high = 7;                                          // corner codes of the edge's two path corners
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if ((int)(edge >> 2) == c) low = tsdf_tet_corner(tau, c);
          if ((int)(edge & 3u) == c) high = tsdf_tet_corner(tau, c);
        }
        const int owner = o + (low & 1) + ((low >> 1 & 1) + (low >> 2) * g.ny) * g.nx;
        const int dir = high ^ low;
        const int type = dir == 1 ? 0 : dir == 2 ? 1 : dir == 4 ? 2 : dir == 3 ? 3 : dir == 5 ? 4 : dir == 6 ? 5 : 6;
        index[v] = vertex_scan[owner] + __popc((uint32_t)word[owner] & ((1u << type) - 1u));
      }
      const bool mirrored = tsdf_tet_mirrored(tau);
      out_faces[face * 3 + 0] = index[0];
      out_faces[face * 3 + 1] = mirrored ? index[2] : index[1];
      out_faces[face * 3 + 2] = mirrored ? index[1] : index[2];
      ++face;
    }
  }
}

static bool tsdf_grid_ok(int nx, int ny, int nz) {
  return nx >= 1 && ny >= 1 && nz >= 1 && (int64_t)nx * ny * nz <= MS_TSDF_MAX_SAMPLES;
}

static TsdfGrid tsdf_grid(int nx, int ny, int nz, const double* origin, double voxel_size) {
  TsdfGrid g;
  g.nx = nx; g.ny = ny; g.nz = nz;
  g.ox = (float)origin[0]; g.oy = (float)origin[1]; g.oz = (float)origin[2];
  g.voxel = (float)voxel_size;
  return g;
}

}  // namespace ms

using namespace ms;

extern "C" int ms_tsdf_integrate(float* tsdf, float* weight, float* colour, int nx, int ny, int nz, const double* origin_host,
                                 double voxel_size, double truncation, double max_weight, const float* depth,
                                 const float* pixel_weight, const float* image, const float* cameras, int num_cameras,
                                 int width, int height, void* stream) {
  MS_CHECK_ARG(tsdf_grid_ok(nx, ny, nz), "dims >= 1 with nx ny nz <= 2^27 expected");
  MS_CHECK_ARG(origin_host != nullptr, "null origin");
  MS_CHECK_ARG(voxel_size > 0.0 && voxel_size < 1e30, "voxel_size > 0 expected");
  MS_CHECK_ARG(truncation > 0.0 && truncation < 1e30, "truncation > 0 expected");
  MS_CHECK_ARG(max_weight > 0.0, "max_weight > 0 expected (infinity: no clamp)");
  MS_CHECK_ARG(num_cameras >= 1 && num_cameras <= MS_COVERAGE_MAX_CAMERAS, "1 <= num_cameras <= 65535 expected");
  MS_CHECK_ARG(width >= 1 && height >= 1 && (int64_t)width * height < ((int64_t)1 << 31), "image of 1 .. 2^31 - 1 pixels expected");
  MS_CHECK_ARG(tsdf && weight && depth && cameras, "null tsdf, weight, depth or cameras");
  MS_CHECK_ARG((colour == nullptr) == (image == nullptr), "a coloured volume needs colour images, a plain one takes none");
  MS_CHECK_ARG(aligned(16, {tsdf, weight, colour}), "tsdf, weight and colour must be aligned to 16 bytes");
  MS_CHECK_ARG(aligned(4, {depth, pixel_weight, image, cameras}), "depth, pixel_weight, image and cameras must be aligned to 4 bytes");
  const int n = nx * ny * nz;
  const TsdfGrid g = tsdf_grid(nx, ny, nz, origin_host, voxel_size);
  tsdf_integrate_kernel<<<dim3((unsigned)div_up(div_up(n, TSDF_RUN), 256)), dim3(256), 0, (hipStream_t)stream>>>(
      tsdf, weight, colour, g, n, (float)truncation, (float)max_weight, depth, pixel_weight, image, cameras, num_cameras,
      width, height);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_tsdf_classify(const float* tsdf, const float* weight, int nx, int ny, int nz, double min_weight,
                                int32_t* word, int32_t* vertex_count, int32_t* triangle_count, void* stream) {
  MS_CHECK_ARG(tsdf_grid_ok(nx, ny, nz), "dims >= 1 with nx ny nz <= 2^27 expected");
  MS_CHECK_ARG(min_weight == min_weight, "NaN min_weight");
  MS_CHECK_ARG(tsdf && weight && word && vertex_count && triangle_count, "null pointer");
  MS_CHECK_ARG(aligned(4, {tsdf, weight, word, vertex_count, triangle_count}), "every pointer must be aligned to 4 bytes");
  const int n = nx * ny * nz;
  const double zero[3] = {0.0, 0.0, 0.0};
  tsdf_classify_kernel<<<dim3((unsigned)div_up(n, 256)), dim3(256), 0, (hipStream_t)stream>>>(
      tsdf, weight, tsdf_grid(nx, ny, nz, zero, 1.0), n, (float)min_weight, word, vertex_count, triangle_count);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_tsdf_emit(const float* tsdf, const float* weight, const float* colour, int nx, int ny, int nz,
                            const double* origin_host, double voxel_size, double min_weight, const int32_t* word,
                            const int32_t* vertex_scan, const int32_t* triangle_scan, float* out_vertices,
                            int32_t* out_faces, float* out_colours, void* stream) {
  MS_CHECK_ARG(tsdf_grid_ok(nx, ny, nz), "dims >= 1 with nx ny nz <= 2^27 expected");
  MS_CHECK_ARG(origin_host != nullptr, "null origin");
  MS_CHECK_ARG(voxel_size > 0.0 && voxel_size < 1e30, "voxel_size > 0 expected");
  MS_CHECK_ARG(min_weight == min_weight, "NaN min_weight");
  MS_CHECK_ARG(tsdf && weight && word && vertex_scan && triangle_scan, "null pointer");
  MS_CHECK_ARG(out_vertices && out_faces, "null output (an empty mesh needs no emit call)");
  MS_CHECK_ARG(out_colours == nullptr || colour != nullptr, "out_colours needs a coloured volume");
  MS_CHECK_ARG(aligned(4, {tsdf, weight, colour, word, vertex_scan, triangle_scan, out_vertices, out_faces, out_colours}),
               "every pointer must be aligned to 4 bytes");
  const int n = nx * ny * nz;
  tsdf_emit_kernel<<<dim3((unsigned)div_up(n, 256)), dim3(256), 0, (hipStream_t)stream>>>(
      tsdf, weight, colour, tsdf_grid(nx, ny, nz, origin_host, voxel_size), n, (float)min_weight, word, vertex_scan,
      triangle_scan, out_vertices, out_faces, out_colours);
  MS_CHECK_LAUNCH();
  return 0;
}
