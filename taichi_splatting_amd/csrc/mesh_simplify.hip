// mesh_simplify.hip — mesh simplification by vertex clustering (Rossignac & Borrel 1993) with the quadric-error
// representative of Lindstrom, "Out-of-core simplification of large polygonal models" (SIGGRAPH 2000), per grid cell (no
// reference counterpart: an addition; what 2DGS, GOF and PGSR leave to Open3D).  A sort, two scans and a per-cluster
// reduction: no edge-collapse queue, no atomics on floats, bitwise reproducible.  The CELL RULE, ORDER RULE, FACE RULE and
// PLACEMENT RULE are stated in include/mi355_splat.h; tests/mesh_simplify_oracle.py holds them in numpy.
// Kernels of this file = 11 (tests/test_mesh_simplify_budgets.py holds the count, 0 bytes of scratch and the registers).
//
// No entry point of this file takes a scratch block: every array is the caller's, and the caller (mesh.py) runs
// ms_radix_sort_pairs, ms_exclusive_scan_i32 and ms_find_ranges between the calls.  In call order:
//   simplify_origin_kernel    the default origin: the smallest finite coordinate per axis (integer atomics on float bits).
//   simplify_mark_kernel      one lane per face: a face with an index outside 0 .. V - 1 sets MS_MESH_BAD_INDEX and does
//     nothing else; otherwise it stores 1 into `referenced` of its three corners (plain stores of one value).
//   simplify_keys_kernel      one lane per vertex: the 64 bit cell key z << 42 | y << 21 | x of a referenced vertex, the
//     sentinel 2^64 - 1 (it sorts last) for an unreferenced one or one whose cell is not valid — which also sets
//     MS_MESH_NOT_FINITE or MS_MESH_CELL_RANGE; value = the vertex index.
//   (stable 64 bit radix sort: within a cell the order is ascending vertex index)
//   simplify_heads_kernel     flag[i] = the sorted key i starts a run of a real cell.
//   (exclusive scan of the flags: the cluster id of a head, and at [V] the cluster count K)
//   simplify_clusters_kernel  cluster id per vertex (-1: none), member_begin[c] per cluster and member_begin[K] = the
//     number of clustered vertices; lane 0 writes head = (K, status) for the caller's host read.
//   simplify_corner_keys_kernel  (cluster, corner) pair of each of the 3 T corners.
//   (stable 32 bit radix sort on the cluster bits + ms_find_ranges: each cluster's corners in ascending corner order)
//   simplify_place_kernel     THE HOT PATH: SIMPLIFY_GROUP = 16 lanes (one DPP row) per cluster.  Lane j of the group takes
//     the entries j, j + 16, j + 32, .. of the cluster's member run and then of its corner run — the split depends on the
//     run's length alone — and adds them in that order into float64 partials; the 16 partials are combined by a fixed xor
//     butterfly of four DPP steps (quad_perm 1-0-3-2, quad_perm 2-3-0-1, row_half_mirror, row_mirror).  An IEEE sum
//     commutes, so after every step the two partners hold the same bits and all 16 lanes end with one value that does
//     not depend on launch order.  Means, quadric, the closed-form 3 x 3 solve, the in-cell test and the fallbacks are
//     then evaluated by every lane alike; lane 0 of the group writes.  No LDS, no scratch, the system in named scalars,
//     every loop bounded by its range length.
//   simplify_faces_kernel     rewrites a face to its corners' clusters, rotates the smallest first, writes the sort key of
//     the first de-duplication pass (the third index) and keep = 0 for a face with two equal corners.
//   simplify_pair_keys_kernel the key first << shift | second of the second pass, in the order the first pass left.
//   (two stable sorts: equal triples end up adjacent, in ascending face index)
//   simplify_dedup_kernel     keeps a face with three different corners whose triple differs from its predecessor's and
//     scatters the flag by face index.
//   simplify_map_kernel       vertex_map[v] = the output vertex of v's cluster after ms_mesh_select_plan's compaction, or -1.
#pragma clang fp contract(off)
#include "mesh_internal.h"

namespace ms {

constexpr int SIMPLIFY_GROUP = 16;                                  // lanes per cluster of simplify_place_kernel: one DPP row
constexpr int SIMPLIFY_CELL_BITS = 21;
constexpr uint64_t SIMPLIFY_NO_CELL = ~(uint64_t)0;
constexpr float SIMPLIFY_LAST_CELL = (float)MS_MESH_SIMPLIFY_MAX_CELL;

// CELL RULE, one axis: one IEEE subtraction, one correctly rounded division, one floor.  The division is carried out in
// float64 and rounded to float32: 53 >= 2 * 24 + 2 bits make that double rounding exact, whatever the compiler's float32
// division is.  The result is a whole number, an infinity or a NaN.
__device__ __forceinline__ float simplify_cell_axis(float p, float origin, float cell_size) {
  const float d = p - origin;
  return floorf((float)((double)d / (double)cell_size));
}
__device__ __forceinline__ bool simplify_cell_valid(float q) { return q >= 0.f && q <= SIMPLIFY_LAST_CELL; }   // false for a NaN

// key of a position, or SIMPLIFY_NO_CELL when an axis leaves 0 .. 2^21 - 1 (or is not a number)
__device__ __forceinline__ uint64_t simplify_cell_key(float x, float y, float z, float ox, float oy, float oz, float cell_size) {
  const float qx = simplify_cell_axis(x, ox, cell_size), qy = simplify_cell_axis(y, oy, cell_size),
              qz = simplify_cell_axis(z, oz, cell_size);
  if (!(simplify_cell_valid(qx) && simplify_cell_valid(qy) && simplify_cell_valid(qz))) return SIMPLIFY_NO_CELL;
  return ((uint64_t)(uint32_t)qz << (2 * SIMPLIFY_CELL_BITS)) | ((uint64_t)(uint32_t)qy << SIMPLIFY_CELL_BITS) | (uint64_t)(uint32_t)qx;
}

__device__ __forceinline__ bool simplify_finite(double v) { return v - v == 0.0; }

// The default origin: the smallest finite coordinate per axis, under the total order in which -0 lies below +0
// (simplify_below), so that the BITS of the result do not depend on any order either.  A lane walks a grid-stride run, the
// wave combines, and lane 0 commits with INTEGER atomics on the float's bits, chosen by the SIGN BIT: a pattern without
// it by a signed minimum, a pattern with it (-0 included) by an unsigned maximum.  Patterns without the sign bit order
// as signed integers; patterns with it order inversely as unsigned integers, lie above every pattern without it as
// unsigned and below it as signed.  So whatever the order of the commits: a signed minimum never replaces a stored
// negative (it is below as signed), an unsigned maximum always replaces a stored non-negative, and 0x80000000 = -0 beats
// every non-negative pattern and loses to every other negative one.  origin starts at +infinity.
__device__ __forceinline__ bool simplify_below(float a, float b) {
  return a < b || (a == b && __float_as_int(a) < 0 && __float_as_int(b) >= 0);
}
__global__ void __launch_bounds__(256)
simplify_origin_kernel(const float* __restrict__ vertices, int64_t num_vertices, float* __restrict__ origin) {
  const float huge = __builtin_huge_valf();
  float low[3] = {huge, huge, huge};
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < num_vertices; v += stride) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float x = vertices[v * 3 + k];
      if (simplify_below(x, low[k]) && x > -huge) low[k] = x;        // false for a NaN
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float x = wave_all(low[k], [](float x, float y) { if (simplify_below(y, x)) x = y; return x; });
    // a wave that cannot lower the value it sees stays out: the stored value only ever falls in that order, so a commit
    // that is skipped would have changed nothing.  The load is a filter only; the atomics alone decide.
    const float seen = __hip_atomic_load(origin + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane_id() == 0 && simplify_below(x, seen)) {
      if (__float_as_int(x) >= 0) atomicMin(reinterpret_cast<int*>(origin + k), __float_as_int(x));
      else atomicMax(reinterpret_cast<unsigned int*>(origin + k), __float_as_uint(x));
    }
  }
}

__global__ void __launch_bounds__(256)
simplify_mark_kernel(const int32_t* __restrict__ faces, int32_t num_vertices, int64_t num_faces,
                     int32_t* __restrict__ referenced, int32_t* __restrict__ status) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= num_faces) return;
  const int32_t a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
  if (!mesh_in_range(a, b, c, num_vertices)) {
    atomicOr(status, MS_MESH_BAD_INDEX);
    return;
  }
  referenced[a] = 1;
  referenced[b] = 1;
  referenced[c] = 1;
}

__global__ void __launch_bounds__(256)
simplify_keys_kernel(const float* __restrict__ vertices, int32_t num_vertices, const int32_t* __restrict__ referenced,
                     const float* __restrict__ origin, float cell_size, uint64_t* __restrict__ keys,
                     int32_t* __restrict__ values, int32_t* __restrict__ status) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= num_vertices) return;
  uint64_t key = SIMPLIFY_NO_CELL;
  if (referenced[v] != 0) {
    const float x = vertices[v * 3 + 0], y = vertices[v * 3 + 1], z = vertices[v * 3 + 2];
    key = simplify_cell_key(x, y, z, origin[0], origin[1], origin[2], cell_size);
    if (key == SIMPLIFY_NO_CELL) {
      const bool finite = simplify_finite((double)x) && simplify_finite((double)y) && simplify_finite((double)z);
      atomicOr(status, finite ? MS_MESH_CELL_RANGE : MS_MESH_NOT_FINITE);
    }
  }
  keys[v] = key;
  values[v] = (int32_t)v;
}

__global__ void __launch_bounds__(256)
simplify_heads_kernel(const uint64_t* __restrict__ sorted_keys, int32_t num_vertices, int32_t* __restrict__ head_flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= num_vertices) return;
  const uint64_t key = sorted_keys[i];
  head_flag[i] = (key != SIMPLIFY_NO_CELL && (i == 0 || sorted_keys[i - 1] != key)) ? 1 : 0;
}

__global__ void __launch_bounds__(256)
simplify_clusters_kernel(const uint64_t* __restrict__ sorted_keys, const int32_t* __restrict__ sorted_vertices,
                         const int32_t* __restrict__ head_scan, int32_t num_vertices, int32_t* __restrict__ vertex_cluster,
                         int32_t* __restrict__ member_begin, const int32_t* __restrict__ status, int32_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > num_vertices) return;
  const int32_t before = head_scan[i];                               // heads in front of i; [V] = K
  if (i == 0) {
    head[0] = head_scan[num_vertices];
    head[1] = *status;
  }
  const uint64_t key = i < num_vertices ? sorted_keys[i] : SIMPLIFY_NO_CELL;
  const uint64_t previous = i > 0 ? sorted_keys[i - 1] : SIMPLIFY_NO_CELL;
  if (key == SIMPLIFY_NO_CELL) {
    if (i == 0 || previous != SIMPLIFY_NO_CELL) member_begin[before] = (int32_t)i;      // the end of the last cluster
  } else if (i == 0 || previous != key) {
    member_begin[before] = (int32_t)i;
  }
  if (i < num_vertices) {
    const int32_t v = sorted_vertices[i];
    if ((uint32_t)v < (uint32_t)num_vertices)
      vertex_cluster[v] = key == SIMPLIFY_NO_CELL ? -1 : ((i == 0 || previous != key) ? before : before - 1);
  }
}

__global__ void __launch_bounds__(256)
simplify_corner_keys_kernel(const int32_t* __restrict__ faces, int32_t num_vertices, int64_t num_corners,
                            const int32_t* __restrict__ vertex_cluster, int32_t num_clusters, uint32_t* __restrict__ keys,
                            int32_t* __restrict__ values) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= num_corners) return;
  const int32_t v = faces[i];
  const int32_t c = (uint32_t)v < (uint32_t)num_vertices ? vertex_cluster[v] : -1;
  keys[i] = (uint32_t)c < (uint32_t)num_clusters ? (uint32_t)c : (uint32_t)num_clusters;      // behind every cluster
  values[i] = (int32_t)i;
}

// the test of the PLACEMENT RULE: is the rounded position inside the cluster's own cell?
__device__ __forceinline__ bool simplify_inside(float x, float y, float z, float ox, float oy, float oz, float cell_size,
                                                uint64_t key) {
  return simplify_cell_key(x, y, z, ox, oy, oz, cell_size) == key;     // key is a real cell: never SIMPLIFY_NO_CELL
}

__global__ void __launch_bounds__(256)
simplify_place_kernel(const float* __restrict__ vertices, const float* __restrict__ colours, const int32_t* __restrict__ faces,
                      int32_t num_vertices, int64_t num_corners, const float* __restrict__ origin, float cell_size,
                      double regularisation, int quadric, const uint64_t* __restrict__ sorted_keys,
                      const int32_t* __restrict__ sorted_vertices, const int32_t* __restrict__ member_begin,
                      int32_t num_clusters, const int32_t* __restrict__ corner_ranges,
                      const int32_t* __restrict__ sorted_corners, float* __restrict__ out_vertices,
                      float* __restrict__ out_colours, uint8_t* __restrict__ out_choice) {
  const int sub = (int)(threadIdx.x & (SIMPLIFY_GROUP - 1));
  const int64_t cluster = (int64_t)blockIdx.x * (256 / SIMPLIFY_GROUP) + (threadIdx.x / SIMPLIFY_GROUP);
  const bool live = cluster < num_clusters;                          // a dead group walks empty ranges: no lane leaves early
  int64_t begin = 0, end = 0;
  if (live) {
    begin = member_begin[cluster];
    end = member_begin[cluster + 1];
    if (begin < 0) begin = 0;
    if (end > num_vertices) end = num_vertices;
  }
  // pass 1: the float64 sums of the member positions (and colours)
  double sx = 0.0, sy = 0.0, sz = 0.0, cr = 0.0, cg = 0.0, cb = 0.0;
  for (int64_t i = begin + sub; i < end; i += SIMPLIFY_GROUP) {
    const int32_t v = sorted_vertices[i];
    if ((uint32_t)v >= (uint32_t)num_vertices) continue;
    sx += (double)vertices[(int64_t)v * 3 + 0];
    sy += (double)vertices[(int64_t)v * 3 + 1];
    sz += (double)vertices[(int64_t)v * 3 + 2];
    if (colours) {
      cr += (double)colours[(int64_t)v * 3 + 0];
      cg += (double)colours[(int64_t)v * 3 + 1];
      cb += (double)colours[(int64_t)v * 3 + 2];
    }
  }
  sx = row_sum16(sx);
  sy = row_sum16(sy);
  sz = row_sum16(sz);
  if (colours) {                                                     // uniform over the launch
    cr = row_sum16(cr);
    cg = row_sum16(cg);
    cb = row_sum16(cb);
  }
  const double members = (double)(end > begin ? end - begin : 1);
  const double mx = sx / members, my = sy / members, mz = sz / members;

  // pass 2: A = sum m m^T, r = sum d m over the cluster's corners, m = (b - a) x (c - a), d = -m . (a - mean)
  double axx = 0.0, axy = 0.0, axz = 0.0, ayy = 0.0, ayz = 0.0, azz = 0.0, rx = 0.0, ry = 0.0, rz = 0.0;
  if (quadric) {                                                     // uniform over the launch
    int64_t first = 0, last = 0;
    if (live) {
      first = corner_ranges[cluster * 2 + 0];
      last = corner_ranges[cluster * 2 + 1];
      if (first < 0) first = 0;
      if (last > num_corners) last = num_corners;
    }
    for (int64_t i = first + sub; i < last; i += SIMPLIFY_GROUP) {
      const int32_t corner = sorted_corners[i];
      if ((uint32_t)corner >= (uint64_t)num_corners) continue;
      const int64_t f = corner / 3;
      const int32_t a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
      if (!mesh_in_range(a, b, c, num_vertices)) continue;
      const double px = vertices[(int64_t)a * 3 + 0], py = vertices[(int64_t)a * 3 + 1], pz = vertices[(int64_t)a * 3 + 2];
      const double ux = (double)vertices[(int64_t)b * 3 + 0] - px, uy = (double)vertices[(int64_t)b * 3 + 1] - py,
                   uz = (double)vertices[(int64_t)b * 3 + 2] - pz;
      const double wx = (double)vertices[(int64_t)c * 3 + 0] - px, wy = (double)vertices[(int64_t)c * 3 + 1] - py,
                   wz = (double)vertices[(int64_t)c * 3 + 2] - pz;
      const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
      const double d = -(nx * (px - mx) + ny * (py - my) + nz * (pz - mz));
      axx += nx * nx;
      axy += nx * ny;
      axz += nx * nz;
      ayy += ny * ny;
      ayz += ny * nz;
      azz += nz * nz;
      rx += d * nx;
      ry += d * ny;
      rz += d * nz;
    }
    axx = row_sum16(axx);
    axy = row_sum16(axy);
    axz = row_sum16(axz);
    ayy = row_sum16(ayy);
    ayz = row_sum16(ayz);
    azz = row_sum16(azz);
    rx = row_sum16(rx);
    ry = row_sum16(ry);
    rz = row_sum16(rz);
  }
  if (!live || sub != 0 || end <= begin) return;                     // the reductions are over: one lane finishes the cluster

  const uint64_t key = sorted_keys[begin];
  const float ox = origin[0], oy = origin[1], oz = origin[2];
  float x = 0.f, y = 0.f, z = 0.f;
  int choice = MS_MESH_SIMPLIFY_MEMBER;
  const double trace = axx + ayy + azz;
  if (quadric && trace > 0.0 && simplify_finite(trace)) {
    // (A + lambda I) y = r by the adjugate: symmetric positive definite, condition number <= 1 + 3 / regularisation
    const double lambda = regularisation * trace / 3.0;
    const double m00 = axx + lambda, m11 = ayy + lambda, m22 = azz + lambda, m01 = axy, m02 = axz, m12 = ayz;
    const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
    const double det = m00 * c00 + m01 * c01 + m02 * c02;
    const double qx = mx - (c00 * rx + c01 * ry + c02 * rz) / det;
    const double qy = my - (c01 * rx + c11 * ry + c12 * rz) / det;
    const double qz = mz - (c02 * rx + c12 * ry + c22 * rz) / det;
    if (simplify_finite(qx) && simplify_finite(qy) && simplify_finite(qz) &&
        simplify_inside((float)qx, (float)qy, (float)qz, ox, oy, oz, cell_size, key)) {
      x = (float)qx;
      y = (float)qy;
      z = (float)qz;
      choice = MS_MESH_SIMPLIFY_QUADRIC;
    }
  }
  if (choice == MS_MESH_SIMPLIFY_MEMBER && simplify_inside((float)mx, (float)my, (float)mz, ox, oy, oz, cell_size, key)) {
    x = (float)mx;
    y = (float)my;
    z = (float)mz;
    choice = MS_MESH_SIMPLIFY_MEAN;
  }
  if (choice == MS_MESH_SIMPLIFY_MEMBER) {                           // the member with the lowest index, bit for bit
    const int32_t v = sorted_vertices[begin];
    if ((uint32_t)v < (uint32_t)num_vertices) {
      x = vertices[(int64_t)v * 3 + 0];
      y = vertices[(int64_t)v * 3 + 1];
      z = vertices[(int64_t)v * 3 + 2];
    }
  }
  out_vertices[cluster * 3 + 0] = x;
  out_vertices[cluster * 3 + 1] = y;
  out_vertices[cluster * 3 + 2] = z;
  if (colours) {
    out_colours[cluster * 3 + 0] = (float)(cr / members);
    out_colours[cluster * 3 + 1] = (float)(cg / members);
    out_colours[cluster * 3 + 2] = (float)(cb / members);
  }
  if (out_choice) out_choice[cluster] = (uint8_t)choice;
}

__global__ void __launch_bounds__(256)
simplify_faces_kernel(const int32_t* __restrict__ faces, int32_t num_vertices, int64_t num_faces,
                      const int32_t* __restrict__ vertex_cluster, int32_t num_clusters, int32_t* __restrict__ out_faces,
                      uint32_t* __restrict__ third_keys, int32_t* __restrict__ values, uint8_t* __restrict__ keep) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= num_faces) return;
  const int32_t a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
  int32_t p = -1, q = -1, r = -1;
  if (mesh_in_range(a, b, c, num_vertices)) {
    p = vertex_cluster[a];
    q = vertex_cluster[b];
    r = vertex_cluster[c];
  }
  const bool kept = mesh_in_range(p, q, r, num_clusters) && p != q && q != r && r != p;
  if (!kept) {
    p = q = r = 0;                                                    // not a triangle: never kept, never read as one
  } else if (q < p && q < r) {                                        // rotate the smallest first: the orientation stays
    const int32_t t = p;
    p = q;
    q = r;
    r = t;
  } else if (r < p && r < q) {
    const int32_t t = r;
    r = q;
    q = p;
    p = t;
  }
  out_faces[f * 3 + 0] = p;
  out_faces[f * 3 + 1] = q;
  out_faces[f * 3 + 2] = r;
  third_keys[f] = (uint32_t)r;
  values[f] = (int32_t)f;
  keep[f] = kept ? 1 : 0;
}

__global__ void __launch_bounds__(256)
simplify_pair_keys_kernel(const int32_t* __restrict__ new_faces, const int32_t* __restrict__ order, int64_t num_faces,
                          int shift, uint64_t* __restrict__ pair_keys) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= num_faces) return;
  const int32_t f = order[i];
  uint64_t key = 0;
  if ((uint32_t)f < (uint64_t)num_faces)
    key = ((uint64_t)(uint32_t)new_faces[(int64_t)f * 3 + 0] << shift) | (uint64_t)(uint32_t)new_faces[(int64_t)f * 3 + 1];
  pair_keys[i] = key;
}

__global__ void __launch_bounds__(256)
simplify_dedup_kernel(const int32_t* __restrict__ new_faces, const int32_t* __restrict__ order, int64_t num_faces,
                      uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < 1 || i >= num_faces) return;
  const int32_t f = order[i], g = order[i - 1];
  if ((uint32_t)f >= (uint64_t)num_faces || (uint32_t)g >= (uint64_t)num_faces) return;
  // g precedes f and holds the same triple: g < f (both sorts are stable), so f is the duplicate.  A face with two equal
  // corners holds (0, 0, 0), which no triangle does.
  if (new_faces[(int64_t)f * 3 + 0] == new_faces[(int64_t)g * 3 + 0] && new_faces[(int64_t)f * 3 + 1] == new_faces[(int64_t)g * 3 + 1] &&
      new_faces[(int64_t)f * 3 + 2] == new_faces[(int64_t)g * 3 + 2])
    keep[f] = 0;
}

__global__ void __launch_bounds__(256)
simplify_map_kernel(const int32_t* __restrict__ vertex_cluster, int32_t num_vertices, const int32_t* __restrict__ cluster_scan,
                    int32_t num_clusters, int32_t* __restrict__ vertex_map) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= num_vertices) return;
  const int32_t c = vertex_cluster[v];
  int32_t to = -1;
  if ((uint32_t)c < (uint32_t)num_clusters && cluster_scan[c + 1] != cluster_scan[c]) to = cluster_scan[c];
  vertex_map[v] = to;
}


}  // namespace ms

using namespace ms;

#define SIMPLIFY_CHECK_SIZES(v, f) \
  MS_CHECK_ARG(mesh_sizes_ok(v, f), "0 <= V <= 2^31 - 1 and 0 <= 3 T <= 2^31 - 1 expected")

extern "C" int ms_mesh_simplify_origin(const float* vertices, int64_t num_vertices, float* origin, void* stream) {
  SIMPLIFY_CHECK_SIZES(num_vertices, 0);
  MS_CHECK_ARG(origin && (vertices || num_vertices == 0), "null origin or vertices");
  MS_CHECK_ARG(aligned(4, {vertices, origin}), "every pointer must be aligned to 4 bytes");
  hipStream_t s = (hipStream_t)stream;
  if (num_vertices == 0) {
    MS_CHECK_HIP(hipMemsetAsync(origin, 0, 3 * sizeof(float), s));
    return 0;
  }
  MS_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)origin, 0x7f800000, 3, s));      // +infinity
  const int64_t blocks = div_up(num_vertices, 256 * 16);                            // 16 vertices a lane, at most 1024 workgroups
  simplify_origin_kernel<<<dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s>>>(vertices, num_vertices, origin);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_mesh_simplify_keys(const float* vertices, const int32_t* faces, int64_t num_vertices, int64_t num_faces,
                                     const float* origin, float cell_size, int32_t* referenced, uint64_t* keys,
                                     int32_t* values, int32_t* status, int32_t* head, void* stream) {
  SIMPLIFY_CHECK_SIZES(num_vertices, num_faces);
  MS_CHECK_ARG(cell_size > 0.f && cell_size < __builtin_huge_valf(), "cell_size must be a finite positive float32");
  MS_CHECK_ARG(status && head && origin, "null status, head or origin");
  MS_CHECK_ARG((vertices && referenced && keys && values) || num_vertices == 0, "null vertices, referenced, keys or values");
  MS_CHECK_ARG(faces || num_faces == 0, "null faces");
  MS_CHECK_ARG(aligned(4, {vertices, faces, origin, referenced, values, status, head}) && aligned(8, {keys}),
               "every pointer must be aligned to 4 bytes, keys to 8");
  hipStream_t s = (hipStream_t)stream;
  MS_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
  MS_CHECK_HIP(hipMemsetAsync(head, 0xff, 2 * sizeof(int32_t), s));        // poisoned until ms_mesh_simplify_clusters ran
  if (num_vertices == 0) {
    if (num_faces > 0) simplify_mark_kernel<<<mesh_grid(num_faces), dim3(256), 0, s>>>(faces, 0, num_faces, nullptr, status);
    MS_CHECK_LAUNCH();
    return 0;
  }
  MS_CHECK_HIP(hipMemsetAsync(referenced, 0, (size_t)num_vertices * 4, s));
  if (num_faces > 0)
    simplify_mark_kernel<<<mesh_grid(num_faces), dim3(256), 0, s>>>(faces, (int32_t)num_vertices, num_faces, referenced, status);
  simplify_keys_kernel<<<mesh_grid(num_vertices), dim3(256), 0, s>>>(vertices, (int32_t)num_vertices, referenced, origin,
                                                                       cell_size, keys, values, status);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_mesh_simplify_heads(const uint64_t* sorted_keys, int64_t num_vertices, int32_t* head_flag, void* stream) {
  SIMPLIFY_CHECK_SIZES(num_vertices, 0);
  MS_CHECK_ARG(head_flag != nullptr, "null head_flag");
  MS_CHECK_ARG(sorted_keys || num_vertices == 0, "null sorted_keys");
  MS_CHECK_ARG(aligned(4, {head_flag}) && aligned(8, {sorted_keys}), "head_flag aligned to 4 bytes, sorted_keys to 8");
  if (num_vertices == 0) return 0;
  simplify_heads_kernel<<<mesh_grid(num_vertices), dim3(256), 0, (hipStream_t)stream>>>(sorted_keys, (int32_t)num_vertices, head_flag);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_mesh_simplify_clusters(const uint64_t* sorted_keys, const int32_t* sorted_vertices, const int32_t* head_scan,
                                         int64_t num_vertices, int32_t* vertex_cluster, int32_t* member_begin,
                                         const int32_t* status, int32_t* head, void* stream) {
  SIMPLIFY_CHECK_SIZES(num_vertices, 0);
  MS_CHECK_ARG(head_scan && member_begin && status && head, "null head_scan, member_begin, status or head");
  MS_CHECK_ARG((sorted_keys && sorted_vertices && vertex_cluster) || num_vertices == 0, "null sorted_keys, sorted_vertices or vertex_cluster");
  MS_CHECK_ARG(aligned(4, {sorted_vertices, head_scan, vertex_cluster, member_begin, status, head}) &&
               aligned(8, {sorted_keys}), "every pointer must be aligned to 4 bytes, sorted_keys to 8");
  simplify_clusters_kernel<<<mesh_grid(num_vertices + 1), dim3(256), 0, (hipStream_t)stream>>>(
      sorted_keys, sorted_vertices, head_scan, (int32_t)num_vertices, vertex_cluster, member_begin, status, head);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_mesh_simplify_corner_keys(const int32_t* faces, int64_t num_vertices, int64_t num_faces,
                                            const int32_t* vertex_cluster, int64_t num_clusters, uint32_t* keys,
                                            int32_t* values, void* stream) {
  SIMPLIFY_CHECK_SIZES(num_vertices, num_faces);
  MS_CHECK_ARG(num_clusters >= 0 && num_clusters <= num_vertices, "0 <= K <= V expected");
  if (num_faces == 0) return 0;
  MS_CHECK_ARG(faces && keys && values && (vertex_cluster || num_vertices == 0), "null pointer");
  MS_CHECK_ARG(aligned(4, {faces, vertex_cluster, keys, values}), "every pointer must be aligned to 4 bytes");
  simplify_corner_keys_kernel<<<mesh_grid(3 * num_faces), dim3(256), 0, (hipStream_t)stream>>>(
      faces, (int32_t)num_vertices, 3 * num_faces, vertex_cluster, (int32_t)num_clusters, keys, values);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_mesh_simplify_place(const float* vertices, const float* colours, const int32_t* faces, int64_t num_vertices,
                                      int64_t num_faces, const float* origin, float cell_size, double regularisation,
                                      int placement, const uint64_t* sorted_keys, const int32_t* sorted_vertices,
                                      const int32_t* member_begin, int64_t num_clusters, const int32_t* corner_ranges,
                                      const int32_t* sorted_corners, float* out_vertices, float* out_colours,
                                      uint8_t* out_choice, void* stream) {
  SIMPLIFY_CHECK_SIZES(num_vertices, num_faces);
  MS_CHECK_ARG(num_clusters >= 0 && num_clusters <= num_vertices, "0 <= K <= V expected");
  MS_CHECK_ARG(cell_size > 0.f && cell_size < __builtin_huge_valf(), "cell_size must be a finite positive float32");
  MS_CHECK_ARG(regularisation > 0.0 && regularisation < __builtin_huge_val(), "regularisation must be finite and > 0");
  MS_CHECK_ARG(placement == MS_MESH_SIMPLIFY_QUADRIC || placement == MS_MESH_SIMPLIFY_MEAN,
               "placement is MS_MESH_SIMPLIFY_QUADRIC or MS_MESH_SIMPLIFY_MEAN");
  if (num_clusters == 0) return 0;
  const bool quadric = placement == MS_MESH_SIMPLIFY_QUADRIC && num_faces > 0;
  MS_CHECK_ARG(vertices && origin && sorted_keys && sorted_vertices && member_begin && out_vertices, "null pointer");
  MS_CHECK_ARG(!quadric || (faces && corner_ranges && sorted_corners), "the quadric placement needs faces, corner_ranges and sorted_corners");
  MS_CHECK_ARG((colours == nullptr) == (out_colours == nullptr), "colours is given together with out_colours");
  MS_CHECK_ARG(aligned(4, {vertices, colours, faces, origin, sorted_vertices, member_begin, corner_ranges, sorted_corners,
                                 out_vertices, out_colours}) && aligned(8, {sorted_keys}),
               "every pointer but out_choice must be aligned to 4 bytes, sorted_keys to 8");
  simplify_place_kernel<<<dim3((unsigned)div_up(num_clusters, 256 / SIMPLIFY_GROUP)), dim3(256), 0, (hipStream_t)stream>>>(
      vertices, colours, faces, (int32_t)num_vertices, 3 * num_faces, origin, cell_size, regularisation, quadric ? 1 : 0,
      sorted_keys, sorted_vertices, member_begin, (int32_t)num_clusters, corner_ranges, sorted_corners, out_vertices, out_colours,
      out_choice);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_mesh_simplify_faces(const int32_t* faces, int64_t num_vertices, int64_t num_faces,
                                      const int32_t* vertex_cluster, int64_t num_clusters, int32_t* out_faces,
                                      uint32_t* third_keys, int32_t* values, uint8_t* keep, void* stream) {
  SIMPLIFY_CHECK_SIZES(num_vertices, num_faces);
  MS_CHECK_ARG(num_clusters >= 0 && num_clusters <= num_vertices, "0 <= K <= V expected");
  if (num_faces == 0) return 0;
  MS_CHECK_ARG(faces && out_faces && third_keys && values && keep && (vertex_cluster || num_vertices == 0), "null pointer");
  MS_CHECK_ARG(aligned(4, {faces, vertex_cluster, out_faces, third_keys, values}), "every pointer but keep must be aligned to 4 bytes");
  simplify_faces_kernel<<<mesh_grid(num_faces), dim3(256), 0, (hipStream_t)stream>>>(
      faces, (int32_t)num_vertices, num_faces, vertex_cluster, (int32_t)num_clusters, out_faces, third_keys, values, keep);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_mesh_simplify_pair_keys(const int32_t* new_faces, const int32_t* order, int64_t num_faces, int shift,
                                          uint64_t* pair_keys, void* stream) {
  SIMPLIFY_CHECK_SIZES(0, num_faces);
  MS_CHECK_ARG(shift >= 1 && shift <= 32, "1 <= shift <= 32 expected");
  if (num_faces == 0) return 0;
  MS_CHECK_ARG(new_faces && order && pair_keys, "null pointer");
  MS_CHECK_ARG(aligned(4, {new_faces, order}) && aligned(8, {pair_keys}), "int32 pointers aligned to 4 bytes, pair_keys to 8");
  simplify_pair_keys_kernel<<<mesh_grid(num_faces), dim3(256), 0, (hipStream_t)stream>>>(new_faces, order, num_faces, shift, pair_keys);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_mesh_simplify_dedup(const int32_t* new_faces, const int32_t* order, int64_t num_faces, uint8_t* keep,
                                      void* stream) {
  SIMPLIFY_CHECK_SIZES(0, num_faces);
  if (num_faces == 0) return 0;
  MS_CHECK_ARG(new_faces && order && keep, "null pointer");
  MS_CHECK_ARG(aligned(4, {new_faces, order}), "new_faces and order must be aligned to 4 bytes");
  simplify_dedup_kernel<<<mesh_grid(num_faces), dim3(256), 0, (hipStream_t)stream>>>(new_faces, order, num_faces, keep);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_mesh_simplify_map(const int32_t* vertex_cluster, int64_t num_vertices, const int32_t* cluster_scan,
                                    int64_t num_clusters, int32_t* vertex_map, void* stream) {
  SIMPLIFY_CHECK_SIZES(num_vertices, 0);
  MS_CHECK_ARG(num_clusters >= 0 && num_clusters <= num_vertices, "0 <= K <= V expected");
  if (num_vertices == 0) return 0;
  MS_CHECK_ARG(vertex_cluster && vertex_map && cluster_scan, "null pointer");
  MS_CHECK_ARG(aligned(4, {vertex_cluster, cluster_scan, vertex_map}), "every pointer must be aligned to 4 bytes");
  simplify_map_kernel<<<mesh_grid(num_vertices), dim3(256), 0, (hipStream_t)stream>>>(
      vertex_cluster, (int32_t)num_vertices, cluster_scan, (int32_t)num_clusters, vertex_map);
  MS_CHECK_LAUNCH();
  return 0;
}
