// mesh.hip — mesh clean-up on the index buffer: connected components, face selection with vertex compaction, and
// area-weighted vertex normals (no reference counterpart: an addition; what 2DGS, GOF and PGSR do to an extracted mesh
// before anyone looks at it).  vertices (V, 3) float32, faces (T, 3) int32; faces are connected through shared vertex
// INDICES only, never through coinciding positions.  V <= 2^31 - 1 and 3 T <= 2^31 - 1.
// Kernels of this file = 13 (tests/test_mesh_budgets.py holds the count, 0 bytes of scratch and the registers).
//
// Components (ms_mesh_components): lock-free union-find on parent[V], as in ECL-CC (Jaiganesh & Burtscher, HPDC 2018).
//   mesh_init_kernel     parent[v] = v, vertex_label[v] = -1 (= "no face references v yet").
//   mesh_hook_kernel     one lane per face.  A face with an index outside 0 .. V - 1 sets MS_MESH_BAD_INDEX in the status
//     word and does nothing else: nothing is read or written through it.  Otherwise it stores 0 into vertex_label of its
//     three corners (plain stores of one value) and unites (a, b) and (b, c): find both roots, hook the LARGER root under
//     the smaller with a compare-and-swap on parent[larger] that expects `larger` itself, and after a failed swap find
//     again from the value the swap returned.  Invariants: parent[v] <= v always, so a walk strictly descends and takes
//     fewer than V steps (the loop is bounded by V all the same); only a root is ever the target of a swap, and a vertex
//     that stopped being a root never becomes one again, so the path halving a walk does (plain stores of an ancestor into
//     a non-root) cannot collide with a hook.  No lane waits for another lane's store: a failed swap means another hook
//     succeeded on that root, the retry starts from the new parent, and the larger of the two roots a lane holds strictly
//     decreases from retry to retry.  Retries are capped at MESH_HOOK_RETRIES; a lane that runs out sets MS_MESH_GAVE_UP.
//     Whatever the timing, the final root of a component is its smallest vertex index: that is what makes the labels
//     reproducible although this kernel uses atomics.
//   mesh_flatten_kernel  parent[v] = root of v; rank input[v] = 1 iff v is a referenced root.
//   (ms_exclusive_scan_i32 of the root flags: the dense rank, ascending in the root's = the smallest vertex's index.)
//   mesh_label_kernel    vertex_label[v] = rank[parent[v]] or -1 (unreferenced); face_label[f] = label of its first
//     corner (-1 for a face with a bad index); lane 0 writes head = (K, status) for the caller's one host read.
//   mesh_count_kernel    counts per label: a wave walks MESH_COUNT_CHUNKS = 32 chunks of 64 consecutive labels; the lanes
//     of a chunk that hold the same label combine (ballot + popcount, at most 64 rounds, wave-uniform) and join the run
//     the wave carries in a register pair (label, count); a run is added to its counter, with ONE integer add, only when
//     another label follows it or the wave ends — the common case is one component that holds nearly everything, i.e.
//     one add per 2048 labels (one per lane, and then one per wave and chunk, both measured slower: DESIGN.md §4).
//     Integer adds commute: reproducible.
//
// Filter (ms_mesh_component_filter): mesh_filter_keys_kernel makes (0xffffffff - face_count, label) pairs of the
//   components with face_count >= min_faces (0xffffffff for the others), the stable ms_radix_sort_pairs orders them by
//   descending count with ties in ascending label, mesh_filter_take_kernel flags the first keep_largest, and
//   mesh_filter_mask_kernel turns the per-component flags into the (T,) face mask.
//
// Selection (ms_mesh_select_plan / ms_mesh_select_gather): mesh_mark_kernel stores 1 for every vertex a kept face
//   references (plain stores of one value) and the mask as int32; two exclusive scans; mesh_head_kernel gathers
//   (V', T', status) for the one host read; mesh_gather_kernel moves vertex rows, colours and normals bit for bit to
//   vertex_scan[v] and rewrites the kept faces' indices at face_scan[f]: both orders are the input's (stable).
//
// Normals (ms_mesh_vertex_normals): no float atomics.  mesh_corner_keys_kernel makes a (vertex, corner) pair of each of
//   the 3 T corners (key V for a corner with a bad index: it sorts behind every vertex), the stable radix sort groups
//   them by vertex in ascending corner order, ms_find_ranges gives each vertex its range, and mesh_normals_kernel, one
//   lane per vertex (consecutive lanes read consecutive ranges), sums (b - a) x (c - a) over its corners' faces IN
//   ASCENDING CORNER ORDER IN FLOAT64 — differences, products and the running sum are double operations on the float32
//   positions, no FMA contraction — and rounds the three sums to float32 once.  The unit normal is the double sum
//   divided by its double length, rounded once; a zero (or non-finite) length gives (0, 0, 0).  A face with an index
//   outside 0 .. V - 1 contributes nothing.  A vertex of very high degree is legal and merely slow (one lane walks it).
#pragma clang fp contract(off)
#include "mesh_internal.h"

namespace ms {

constexpr int MESH_HOOK_RETRIES = 1 << 16;
constexpr int MESH_COUNT_CHUNKS = 32;             // chunks of 64 consecutive labels a wave of mesh_count_kernel walks

__device__ __forceinline__ int32_t mesh_load(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void mesh_store(int32_t* p, int32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Root of x, halving the path on the way.  parent[] strictly descends along a walk: fewer than `limit` = V steps.
__device__ __forceinline__ int32_t mesh_find(int32_t* __restrict__ parent, int32_t x, int32_t limit) {
  int32_t cur = x, p = mesh_load(parent + cur);
  for (int32_t step = 0; p != cur && step < limit; ++step) {
    const int32_t g = mesh_load(parent + p);
    if (g != p) mesh_store(parent + cur, g);       // cur is no root and never will be: no hook targets it
    cur = p;
    p = g;
  }
  return cur;
}

__device__ __forceinline__ bool mesh_unite(int32_t* __restrict__ parent, int32_t a, int32_t b, int32_t limit) {
  int32_t ra = mesh_find(parent, a, limit), rb = mesh_find(parent, b, limit);
  for (int retry = 0; retry < MESH_HOOK_RETRIES; ++retry) {
    if (ra == rb) return true;
    const int32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
    const int32_t old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return true;
    ra = mesh_find(parent, old, limit);             // old < hi: another hook took this root; go on from where it points
    rb = mesh_find(parent, lo, limit);
  }
  return ra == rb;
}

__global__ void __launch_bounds__(256)
mesh_init_kernel(int32_t* __restrict__ parent, int32_t* __restrict__ vertex_label, int32_t num_vertices) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= num_vertices) return;
  parent[v] = (int32_t)v;
  vertex_label[v] = -1;
}

__global__ void __launch_bounds__(256)
mesh_hook_kernel(const int32_t* __restrict__ faces, int32_t num_vertices, int64_t num_faces, int32_t* __restrict__ parent,
                 int32_t* __restrict__ vertex_label, int32_t* __restrict__ status) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= num_faces) return;
  const int32_t a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
  if (!mesh_in_range(a, b, c, num_vertices)) {
    atomicOr(status, MS_MESH_BAD_INDEX);
    return;
  }
  vertex_label[a] = 0;
  vertex_label[b] = 0;
  vertex_label[c] = 0;
  bool done = mesh_unite(parent, a, b, num_vertices);
  done = mesh_unite(parent, b, c, num_vertices) && done;
  if (!done) atomicOr(status, MS_MESH_GAVE_UP);
}

__global__ void __launch_bounds__(256)
mesh_flatten_kernel(int32_t* __restrict__ parent, const int32_t* __restrict__ vertex_label, int32_t num_vertices,
                    int32_t* __restrict__ root_flag) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= num_vertices) return;
  int32_t root = (int32_t)v, p = mesh_load(parent + root);
  for (int32_t step = 0; p != root && step < num_vertices; ++step) {
    root = p;
    p = mesh_load(parent + root);
  }
  if (root != (int32_t)v) mesh_store(parent + v, root);       // a root keeps itself: every store is a true root
  root_flag[v] = (root == (int32_t)v && vertex_label[v] == 0) ? 1 : 0;
}

__global__ void __launch_bounds__(256)
mesh_label_kernel(const int32_t* __restrict__ faces, int32_t num_vertices, int64_t num_faces,
                  const int32_t* __restrict__ parent, const int32_t* __restrict__ rank, int32_t* __restrict__ vertex_label,
                  int32_t* __restrict__ face_label, const int32_t* __restrict__ status, int32_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    head[0] = rank[num_vertices];
    head[1] = *status;
  }
  if (i < num_vertices) vertex_label[i] = vertex_label[i] == 0 ? rank[parent[i]] : -1;
  if (i < num_faces) {
    const int32_t a = faces[i * 3 + 0], b = faces[i * 3 + 1], c = faces[i * 3 + 2];
    face_label[i] = mesh_in_range(a, b, c, num_vertices) ? rank[parent[a]] : -1;
  }
}

__global__ void __launch_bounds__(256)
mesh_count_kernel(const int32_t* __restrict__ label, int64_t n, int32_t num_labels, int32_t* __restrict__ count) {
  const int lane = lane_id();
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t base = wave * (WAVE * MESH_COUNT_CHUNKS);
  int32_t run_label = -1, run_count = 0;                          // wave-uniform: the run of equal labels not yet added
  for (int chunk = 0; chunk < MESH_COUNT_CHUNKS; ++chunk) {
    const int64_t i = base + (int64_t)chunk * WAVE + lane;
    const int32_t mine = i < n ? label[i] : -1;
    bool pending = (uint32_t)mine < (uint32_t)num_labels;
    for (int round = 0; round < WAVE; ++round) {                  // one distinct label leaves per round
      const unsigned long long open = __ballot(pending);
      if (open == 0) break;
      const int32_t lead = __shfl(mine, __builtin_ctzll(open), WAVE);
      const int32_t same = (int32_t)__popcll(__ballot(pending && mine == lead));
      if (lead == run_label) {
        run_count += same;
      } else {
        if (run_count > 0 && lane == 0) atomicAdd(count + run_label, run_count);
        run_label = lead;
        run_count = same;
      }
      if (mine == lead) pending = false;
    }
  }
  if (run_count > 0 && lane == 0) atomicAdd(count + run_label, run_count);
}

__global__ void __launch_bounds__(256)
mesh_filter_keys_kernel(const int32_t* __restrict__ face_count, int32_t num_labels, int64_t min_faces, int keep_all,
                        uint32_t* __restrict__ keys, int32_t* __restrict__ values, int32_t* __restrict__ keep) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= num_labels) return;
  const int32_t faces = face_count[k];
  const bool large = (int64_t)faces >= min_faces;
  keys[k] = large ? 0xffffffffu - (uint32_t)faces : 0xffffffffu;      // min_faces >= 1: a kept key is below 0xffffffff
  values[k] = (int32_t)k;
  keep[k] = (keep_all && large) ? 1 : 0;
}

__global__ void __launch_bounds__(256)
mesh_filter_take_kernel(const uint32_t* __restrict__ sorted_keys, const int32_t* __restrict__ sorted_values, int64_t take,
                        int32_t num_labels, int32_t* __restrict__ keep) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= take || j >= num_labels) return;
  const int32_t k = sorted_values[j];
  if (sorted_keys[j] != 0xffffffffu && (uint32_t)k < (uint32_t)num_labels) keep[k] = 1;
}

__global__ void __launch_bounds__(256)
mesh_filter_mask_kernel(const int32_t* __restrict__ face_label, int64_t num_faces, const int32_t* __restrict__ keep,
                        int32_t num_labels, uint8_t* __restrict__ face_mask) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= num_faces) return;
  const int32_t k = face_label[f];
  face_mask[f] = ((uint32_t)k < (uint32_t)num_labels && keep[k] != 0) ? 1 : 0;
}

__global__ void __launch_bounds__(256)
mesh_mark_kernel(const int32_t* __restrict__ faces, const uint8_t* __restrict__ face_mask, int32_t num_vertices,
                 int64_t num_faces, int32_t* __restrict__ vertex_flag, int32_t* __restrict__ face_flag,
                 int32_t* __restrict__ status) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= num_faces) return;
  const bool kept = face_mask[f] != 0;
  face_flag[f] = kept ? 1 : 0;
  if (!kept) return;
  const int32_t a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
  if (!mesh_in_range(a, b, c, num_vertices)) {
    atomicOr(status, MS_MESH_BAD_INDEX);
    return;
  }
  vertex_flag[a] = 1;
  vertex_flag[b] = 1;
  vertex_flag[c] = 1;
}

__global__ void mesh_head_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, const int32_t* __restrict__ c,
                                 int32_t* __restrict__ head) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    head[0] = *a;
    head[1] = *b;
    head[2] = *c;
  }
}

__global__ void __launch_bounds__(256)
mesh_gather_kernel(const uint32_t* __restrict__ vertices, const uint32_t* __restrict__ colours,
                   const uint32_t* __restrict__ normals, const int32_t* __restrict__ faces,
                   const uint8_t* __restrict__ face_mask, int32_t num_vertices, int64_t num_faces,
                   const int32_t* __restrict__ vertex_scan, const int32_t* __restrict__ face_scan,
                   uint32_t* __restrict__ out_vertices, uint32_t* __restrict__ out_colours, uint32_t* __restrict__ out_normals,
                   int32_t* __restrict__ out_faces) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < num_vertices) {
    const int64_t to = vertex_scan[i];
    if (vertex_scan[i + 1] != (int32_t)to) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        out_vertices[to * 3 + k] = vertices[i * 3 + k];
        if (colours) out_colours[to * 3 + k] = colours[i * 3 + k];
        if (normals) out_normals[to * 3 + k] = normals[i * 3 + k];
      }
    }
  }
  if (i < num_faces && face_mask[i] != 0) {
    const int64_t to = face_scan[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int32_t v = faces[i * 3 + k];
      out_faces[to * 3 + k] = (uint32_t)v < (uint32_t)num_vertices ? vertex_scan[v] : 0;     // (a bad index was reported before)
    }
  }
}

__global__ void __launch_bounds__(256)
mesh_corner_keys_kernel(const int32_t* __restrict__ faces, int32_t num_vertices, int64_t num_corners,
                        uint32_t* __restrict__ keys, int32_t* __restrict__ values) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= num_corners) return;
  const int32_t v = faces[i];
  keys[i] = (uint32_t)v < (uint32_t)num_vertices ? (uint32_t)v : (uint32_t)num_vertices;
  values[i] = (int32_t)i;
}

__global__ void __launch_bounds__(256)
mesh_normals_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int32_t num_vertices,
                    int64_t num_corners, const int32_t* __restrict__ ranges, const int32_t* __restrict__ sorted_corners,
                    float* __restrict__ out_sums, float* __restrict__ out_normals) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= num_vertices) return;
  int64_t begin = ranges[v * 2 + 0], end = ranges[v * 2 + 1];
  if (begin < 0) begin = 0;
  if (end > num_corners) end = num_corners;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int64_t i = begin; i < end; ++i) {
    const int32_t corner = sorted_corners[i];
    if ((uint32_t)corner >= (uint64_t)num_corners) continue;
    const int64_t f = corner / 3;
    const int32_t a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    if (!mesh_in_range(a, b, c, num_vertices)) continue;
    const double ax = vertices[(int64_t)a * 3 + 0], ay = vertices[(int64_t)a * 3 + 1], az = vertices[(int64_t)a * 3 + 2];
    const double ux = (double)vertices[(int64_t)b * 3 + 0] - ax, uy = (double)vertices[(int64_t)b * 3 + 1] - ay,
                 uz = (double)vertices[(int64_t)b * 3 + 2] - az;
    const double wx = (double)vertices[(int64_t)c * 3 + 0] - ax, wy = (double)vertices[(int64_t)c * 3 + 1] - ay,
                 wz = (double)vertices[(int64_t)c * 3 + 2] - az;
    sx += uy * wz - uz * wy;
    sy += uz * wx - ux * wz;
    sz += ux * wy - uy * wx;
  }
  if (out_sums) {
    out_sums[v * 3 + 0] = (float)sx;
    out_sums[v * 3 + 1] = (float)sy;
    out_sums[v * 3 + 2] = (float)sz;
  }
  if (out_normals) {
    const double length = sqrt(sx * sx + sy * sy + sz * sz);
    const bool usable = length > 0.0 && length < __builtin_huge_val();
    out_normals[v * 3 + 0] = usable ? (float)(sx / length) : 0.f;
    out_normals[v * 3 + 1] = usable ? (float)(sy / length) : 0.f;
    out_normals[v * 3 + 2] = usable ? (float)(sz / length) : 0.f;
  }
}

static int mesh_key_bits(int64_t largest) {
  int bits = 1;
  while (bits < 32 && ((int64_t)1 << bits) <= largest) ++bits;
  return bits;
}

// Scratch layouts.  Empty arrays keep one element (the kernels are handed real addresses at every size).
static size_t mesh_some(int64_t n) { return (size_t)(n > 0 ? n : 1); }

struct MeshComponentsTmp { size_t status, parent, rank, scan, scan_bytes, total; };
static MeshComponentsTmp mesh_components_tmp(int64_t v) {
  Carve c;
  MeshComponentsTmp t;
  t.status = c.take(4);
  t.parent = c.take(mesh_some(v) * 4);
  t.rank = c.take((size_t)(v + 1) * 4);
  t.scan_bytes = scan_tmp_size(v);
  t.scan = c.take(t.scan_bytes);
  t.total = c.off;
  return t;
}

struct MeshSelectTmp { size_t status, scan, scan_bytes, total; };
static MeshSelectTmp mesh_select_tmp(int64_t v, int64_t f) {
  Carve c;
  MeshSelectTmp t;
  t.status = c.take(4);
  t.scan_bytes = scan_tmp_size(v > f ? v : f);
  t.scan = c.take(t.scan_bytes);
  t.total = c.off;
  return t;
}

// keys, values and their sorted copies: `count` 4-byte entries each, then `extra` bytes, then the sort's own scratch
struct MeshSortTmp { size_t keys, values, keys_sorted, values_sorted, extra, sort, sort_bytes, total; };
static MeshSortTmp mesh_sort_tmp(int64_t count, size_t extra) {
  const size_t column = mesh_some(count) * 4;
  Carve c;
  MeshSortTmp t;
  t.keys = c.take(column);
  t.values = c.take(column);
  t.keys_sorted = c.take(column);
  t.values_sorted = c.take(column);
  t.extra = c.take(extra);
  t.sort_bytes = sort_tmp_size(count, 4);
  t.sort = c.take(t.sort_bytes);
  t.total = c.off;
  return t;
}
// ms_mesh_component_filter: extra = the keep flags of the k components
static MeshSortTmp mesh_filter_tmp(int64_t k) { return mesh_sort_tmp(k, mesh_some(k) * 4); }
// ms_mesh_vertex_normals: sorts the 3 f corners, extra = the (first, last + 1) corner ranges of the v vertices
static MeshSortTmp mesh_normals_tmp(int64_t v, int64_t f) { return mesh_sort_tmp(3 * f, mesh_some(v) * 8); }

}  // namespace ms

using namespace ms;

extern "C" int ms_mesh_components(const int32_t* faces, int64_t num_vertices, int64_t num_faces, int32_t* vertex_label,
                                  int32_t* face_label, int32_t* head, void* tmp, size_t* tmp_bytes, void* stream) {
  MS_CHECK_ARG(mesh_sizes_ok(num_vertices, num_faces), "0 <= V <= 2^31 - 1 and 0 <= 3 T <= 2^31 - 1 expected");
  const MeshComponentsTmp lay = mesh_components_tmp(num_vertices);
  MS_CHECK_TMP(tmp, tmp_bytes, lay.total);
  MS_CHECK_ARG(aligned(256, {tmp}), "tmp must be aligned to 256 bytes");
  MS_CHECK_ARG(head != nullptr, "head is null");
  MS_CHECK_ARG((faces && face_label) || num_faces == 0, "null faces or face_label");
  MS_CHECK_ARG(vertex_label || num_vertices == 0, "null vertex_label");
  MS_CHECK_ARG(aligned(4, {faces, vertex_label, face_label, head}), "every pointer must be aligned to 4 bytes");
  hipStream_t s = (hipStream_t)stream;
  int32_t* status = at<int32_t>(tmp, lay.status);
  int32_t* parent = at<int32_t>(tmp, lay.parent);
  int32_t* rank = at<int32_t>(tmp, lay.rank);
  const int32_t v = (int32_t)num_vertices;
  MS_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
  MS_CHECK_HIP(hipMemsetAsync(head, 0xff, 2 * sizeof(int32_t), s));        // poisoned: (-1, -1) unless the label kernel ran
  if (num_vertices > 0) mesh_init_kernel<<<mesh_grid(num_vertices), dim3(256), 0, s>>>(parent, vertex_label, v);
  if (num_faces > 0) mesh_hook_kernel<<<mesh_grid(num_faces), dim3(256), 0, s>>>(faces, v, num_faces, parent, vertex_label, status);
  if (num_vertices > 0) mesh_flatten_kernel<<<mesh_grid(num_vertices), dim3(256), 0, s>>>(parent, vertex_label, v, rank);
  MS_CHECK_LAUNCH();
  size_t scan_bytes = lay.scan_bytes;
  const int rc = ms_exclusive_scan_i32(rank, num_vertices, rank, nullptr, at<char>(tmp, lay.scan), &scan_bytes, stream);
  if (rc != 0) return rc;
  mesh_label_kernel<<<mesh_grid(num_vertices > num_faces ? num_vertices : num_faces), dim3(256), 0, s>>>(
      faces, v, num_faces, parent, rank, vertex_label, face_label, status, head);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_mesh_component_counts(const int32_t* vertex_label, int64_t num_vertices, const int32_t* face_label,
                                        int64_t num_faces, int64_t num_components, int32_t* vertex_count,
                                        int32_t* face_count, void* stream) {
  MS_CHECK_ARG(mesh_sizes_ok(num_vertices, num_faces), "0 <= V <= 2^31 - 1 and 0 <= 3 T <= 2^31 - 1 expected");
  MS_CHECK_ARG(num_components >= 0 && num_components <= num_vertices, "0 <= K <= V expected");
  if (num_components == 0) return 0;
  MS_CHECK_ARG(vertex_label && vertex_count && face_count && (face_label || num_faces == 0), "null pointer");
  MS_CHECK_ARG(aligned(4, {vertex_label, face_label, vertex_count, face_count}), "every pointer must be aligned to 4 bytes");
  hipStream_t s = (hipStream_t)stream;
  MS_CHECK_HIP(hipMemsetAsync(vertex_count, 0, (size_t)num_components * 4, s));
  MS_CHECK_HIP(hipMemsetAsync(face_count, 0, (size_t)num_components * 4, s));
  const auto count_grid = [](int64_t n) { return dim3((unsigned)div_up(n, 256 * MESH_COUNT_CHUNKS)); };
  mesh_count_kernel<<<count_grid(num_vertices), dim3(256), 0, s>>>(vertex_label, num_vertices, (int32_t)num_components, vertex_count);
  if (num_faces > 0)
    mesh_count_kernel<<<count_grid(num_faces), dim3(256), 0, s>>>(face_label, num_faces, (int32_t)num_components, face_count);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_mesh_component_filter(const int32_t* face_count, int64_t num_components, int64_t min_faces,
                                        int64_t keep_largest, const int32_t* face_label, int64_t num_faces,
                                        uint8_t* face_mask, void* tmp, size_t* tmp_bytes, void* stream) {
  MS_CHECK_ARG(num_components >= 0 && num_components <= MS_MESH_MAX_VERTICES, "0 <= K <= 2^31 - 1 expected");
  MS_CHECK_ARG(num_faces >= 0 && num_faces <= MS_MESH_MAX_CORNERS / 3, "0 <= 3 T <= 2^31 - 1 expected");
  MS_CHECK_ARG(min_faces >= 1, "min_faces >= 1 expected");
  MS_CHECK_ARG(keep_largest >= 0, "keep_largest >= 1 (or 0: every component) expected");
  const MeshSortTmp lay = mesh_filter_tmp(num_components);
  MS_CHECK_TMP(tmp, tmp_bytes, lay.total);
  MS_CHECK_ARG(aligned(256, {tmp}), "tmp must be aligned to 256 bytes");
  if (num_faces == 0) return 0;
  MS_CHECK_ARG(face_label && face_mask && (face_count || num_components == 0), "null pointer");
  MS_CHECK_ARG(aligned(4, {face_count, face_label}), "face_count and face_label must be aligned to 4 bytes");
  hipStream_t s = (hipStream_t)stream;
  uint32_t* keys = at<uint32_t>(tmp, lay.keys);
  int32_t* values = at<int32_t>(tmp, lay.values);
  uint32_t* keys_sorted = at<uint32_t>(tmp, lay.keys_sorted);
  int32_t* values_sorted = at<int32_t>(tmp, lay.values_sorted);
  int32_t* keep = at<int32_t>(tmp, lay.extra);
  const int32_t k = (int32_t)num_components;
  if (num_components > 0) {
    mesh_filter_keys_kernel<<<mesh_grid(num_components), dim3(256), 0, s>>>(face_count, k, min_faces, keep_largest == 0, keys,
                                                                          values, keep);
    MS_CHECK_LAUNCH();
    if (keep_largest > 0) {
      size_t sort_bytes = lay.sort_bytes;
      const int rc = ms_radix_sort_pairs(keys, values, keys_sorted, values_sorted, num_components, 4, 0, 32,
                                         at<char>(tmp, lay.sort), &sort_bytes, stream);
      if (rc != 0) return rc;
      const int64_t take = keep_largest < num_components ? keep_largest : num_components;
      mesh_filter_take_kernel<<<mesh_grid(take), dim3(256), 0, s>>>(keys_sorted, values_sorted, take, k, keep);
    }
  }
  mesh_filter_mask_kernel<<<mesh_grid(num_faces), dim3(256), 0, s>>>(face_label, num_faces, keep, k, face_mask);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_mesh_select_plan(const int32_t* faces, const uint8_t* face_mask, int64_t num_vertices, int64_t num_faces,
                                   int32_t* vertex_scan, int32_t* face_scan, int32_t* head, void* tmp, size_t* tmp_bytes,
                                   void* stream) {
  MS_CHECK_ARG(mesh_sizes_ok(num_vertices, num_faces), "0 <= V <= 2^31 - 1 and 0 <= 3 T <= 2^31 - 1 expected");
  const MeshSelectTmp lay = mesh_select_tmp(num_vertices, num_faces);
  MS_CHECK_TMP(tmp, tmp_bytes, lay.total);
  MS_CHECK_ARG(aligned(256, {tmp}), "tmp must be aligned to 256 bytes");
  MS_CHECK_ARG(vertex_scan && face_scan && head, "null vertex_scan, face_scan or head");
  MS_CHECK_ARG((faces && face_mask) || num_faces == 0, "null faces or face_mask");
  MS_CHECK_ARG(aligned(4, {faces, vertex_scan, face_scan, head}), "every int32 pointer must be aligned to 4 bytes");
  hipStream_t s = (hipStream_t)stream;
  int32_t* status = at<int32_t>(tmp, lay.status);
  MS_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
  MS_CHECK_HIP(hipMemsetAsync(head, 0xff, 3 * sizeof(int32_t), s));        // poisoned until mesh_head_kernel ran
  MS_CHECK_HIP(hipMemsetAsync(vertex_scan, 0, (size_t)(num_vertices + 1) * 4, s));
  MS_CHECK_HIP(hipMemsetAsync(face_scan, 0, (size_t)(num_faces + 1) * 4, s));
  if (num_faces > 0) {
    mesh_mark_kernel<<<mesh_grid(num_faces), dim3(256), 0, s>>>(faces, face_mask, (int32_t)num_vertices, num_faces, vertex_scan,
                                                               face_scan, status);
    MS_CHECK_LAUNCH();
  }
  size_t scan_bytes = lay.scan_bytes;
  char* scan_tmp = at<char>(tmp, lay.scan);
  int rc = ms_exclusive_scan_i32(vertex_scan, num_vertices, vertex_scan, nullptr, scan_tmp, &scan_bytes, stream);
  if (rc != 0) return rc;
  rc = ms_exclusive_scan_i32(face_scan, num_faces, face_scan, nullptr, scan_tmp, &scan_bytes, stream);
  if (rc != 0) return rc;
  mesh_head_kernel<<<dim3(1), dim3(64), 0, s>>>(vertex_scan + num_vertices, face_scan + num_faces, status, head);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_mesh_select_gather(const float* vertices, const float* colours, const float* normals, const int32_t* faces,
                                     const uint8_t* face_mask, int64_t num_vertices, int64_t num_faces,
                                     const int32_t* vertex_scan, const int32_t* face_scan, float* out_vertices,
                                     float* out_colours, float* out_normals, int32_t* out_faces, void* stream) {
  MS_CHECK_ARG(mesh_sizes_ok(num_vertices, num_faces), "0 <= V <= 2^31 - 1 and 0 <= 3 T <= 2^31 - 1 expected");
  if (num_vertices == 0 && num_faces == 0) return 0;
  MS_CHECK_ARG(vertex_scan && face_scan, "null scan");
  MS_CHECK_ARG((vertices && out_vertices) || num_vertices == 0, "null vertices");
  MS_CHECK_ARG((faces && face_mask && out_faces) || num_faces == 0, "null faces, face_mask or out_faces");
  MS_CHECK_ARG((colours == nullptr) == (out_colours == nullptr) && (normals == nullptr) == (out_normals == nullptr),
               "colours and normals are given together with their outputs");
  MS_CHECK_ARG(aligned(4, {vertices, colours, normals, faces, vertex_scan, face_scan, out_vertices, out_colours, out_normals,
                              out_faces}), "every pointer but face_mask must be aligned to 4 bytes");
  mesh_gather_kernel<<<mesh_grid(num_vertices > num_faces ? num_vertices : num_faces), dim3(256), 0, (hipStream_t)stream>>>(
      (const uint32_t*)vertices, (const uint32_t*)colours, (const uint32_t*)normals, faces, face_mask, (int32_t)num_vertices,
      num_faces, vertex_scan, face_scan, (uint32_t*)out_vertices, (uint32_t*)out_colours, (uint32_t*)out_normals, out_faces);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_mesh_vertex_normals(const float* vertices, const int32_t* faces, int64_t num_vertices, int64_t num_faces,
                                      float* out_sums, float* out_normals, void* tmp, size_t* tmp_bytes, void* stream) {
  MS_CHECK_ARG(mesh_sizes_ok(num_vertices, num_faces), "0 <= V <= 2^31 - 1 and 0 <= 3 T <= 2^31 - 1 expected");
  const MeshSortTmp lay = mesh_normals_tmp(num_vertices, num_faces);
  MS_CHECK_TMP(tmp, tmp_bytes, lay.total);
  MS_CHECK_ARG(aligned(256, {tmp}), "tmp must be aligned to 256 bytes");
  if (num_vertices == 0) return 0;
  MS_CHECK_ARG(vertices && (faces || num_faces == 0), "null vertices or faces");
  MS_CHECK_ARG(out_sums || out_normals, "out_sums and out_normals are both null");
  MS_CHECK_ARG(aligned(4, {vertices, faces, out_sums, out_normals}), "every pointer must be aligned to 4 bytes");
  hipStream_t s = (hipStream_t)stream;
  uint32_t* keys = at<uint32_t>(tmp, lay.keys);
  int32_t* values = at<int32_t>(tmp, lay.values);
  uint32_t* keys_sorted = at<uint32_t>(tmp, lay.keys_sorted);
  int32_t* values_sorted = at<int32_t>(tmp, lay.values_sorted);
  int32_t* ranges = at<int32_t>(tmp, lay.extra);
  const int64_t corners = 3 * num_faces;
  if (corners > 0) {
    mesh_corner_keys_kernel<<<mesh_grid(corners), dim3(256), 0, s>>>(faces, (int32_t)num_vertices, corners, keys, values);
    MS_CHECK_LAUNCH();
    size_t sort_bytes = lay.sort_bytes;
    const int rc = ms_radix_sort_pairs(keys, values, keys_sorted, values_sorted, corners, 4, 0, mesh_key_bits(num_vertices),
                                       at<char>(tmp, lay.sort), &sort_bytes, stream);
    if (rc != 0) return rc;
  }
  const int rc = ms_find_ranges(keys_sorted, corners, 4, 0, num_vertices, ranges, stream);
  if (rc != 0) return rc;
  mesh_normals_kernel<<<mesh_grid(num_vertices), dim3(256), 0, s>>>(vertices, faces, (int32_t)num_vertices, corners, ranges,
                                                                   values_sorted, out_sums, out_normals);
  MS_CHECK_LAUNCH();
  return 0;
}
