// densify.hip — the densification step of the training loop: prune and split the rows of every per-point array
// (parameters, optimiser moments, running visibility, total weight) in a fixed launch sequence.  Replaces the torch
// chain of the reference — params[mask] (a nonzero + one gather per tensor and per state tensor) followed by one
// torch.cat per tensor (optim/parameter_class.py:215-248, examples/fit_image_gaussians.py:190-231) — and the child
// geometry of misc/renderer2d.py:36-131; the 3-D split has no counterpart there.
//
// Sequence (one stream, one host read):
//   plan   flags -> ONE exclusive scan over [keep flags | split flags] (ms_exclusive_scan_i32's kernels) -> counts,
//          on the device and in a pinned host word block; the host reads n_out to size the outputs;
//   table  source row and child slot of every destination row
//          ([kept rows in storage order | children grouped by parent], the layout of torch.cat([x[keep], children]));
//   move   ONE launch for every array: a workgroup takes 256 consecutive destination rows through all arrays, so the
//          table is read once per row (into LDS).  The destination of a block is ONE contiguous byte range per array:
//          lanes walk it in 16-byte pieces (rows that are multiples of 16 bytes on 16-byte aligned bases) or 4-byte
//          pieces, fully coalesced stores; loads are coalesced wherever source rows are consecutive (runs of kept rows);
//   split  child geometry in place on the tail rows, which the move filled with copies of their parents.
// HBM traffic: row_bytes read + row_bytes written per destination row and array (zero-filled child rows: written only)
// + 8 bytes of table.
#include "common.h"

namespace ms {

constexpr int32_t CHILD_BIT = ROW_FLAG_BIT;     // LDS encoding of a table row: source row | CHILD_BIT, or -1 (write zeros)

// keep = !(prune | split), split = split & !prune, as int32 for the scan: out[i] = keep, out[n + i] = split
__global__ void __launch_bounds__(256)
densify_flags_kernel(const uint8_t* __restrict__ prune, const uint8_t* __restrict__ split, int64_t n,
                     int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool p = prune[i] != 0, s = split[i] != 0;
  out[i] = (!p && !s) ? 1 : 0;
  out[n + i] = (s && !p) ? 1 : 0;
}

__global__ void densify_counts_kernel(const int32_t* __restrict__ scan, int64_t n, int children,
                                      int32_t* __restrict__ counts, int32_t* __restrict__ counts_host) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int32_t n_kept = scan[n], n_split = scan[2 * n] - n_kept;
  const int32_t c[4] = {n_kept, n_split, n_kept + children * n_split, (int32_t)n};
  for (int k = 0; k < 4; ++k) {
    counts[k] = c[k];
    if (counts_host) counts_host[k] = c[k];
  }
}

__global__ void __launch_bounds__(256)
densify_table_kernel(const int32_t* __restrict__ scan, int64_t n, int children, int64_t n_out,
                     int32_t* __restrict__ src_row, int32_t* __restrict__ child_slot) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t k0 = scan[i], k1 = scan[i + 1];
  if (k1 > k0) {
    if (k0 >= 0 && k0 < n_out) { src_row[k0] = (int32_t)i; child_slot[k0] = -1; }
    return;
  }
  const int32_t s0 = scan[n + i], s1 = scan[n + i + 1];
  if (s1 > s0) {
    const int64_t n_kept = scan[n];
    const int64_t base = n_kept + (int64_t)(s0 - n_kept) * children;
    for (int c = 0; c < children; ++c) {
      const int64_t dst = base + c;
      if (dst >= 0 && dst < n_out) { src_row[dst] = (int32_t)i; child_slot[dst] = c; }
    }
  }
}

struct MoveArray {
  const char* src;
  char* dst;
  uint32_t row_pieces;               // pieces (of 16 or 4 bytes) per row
  uint32_t flags;                    // bit 0: child rows copy the parent, bit 1: 16-byte pieces
};

struct MoveArgs {
  const int32_t* src_row;
  const int32_t* child_slot;
  int64_t n_src, n_out;
  int num_arrays;
  MoveArray a[ROW_MAX_ARRAYS];
};

// The move keeps uint32_t / uint4 as its pieces: with piece4 / piece16 of rows.h the compiler schedules
// densify_move_kernel differently (one instruction more).
template <> __device__ __forceinline__ uint4 zero_piece<uint4>() { return make_uint4(0u, 0u, 0u, 0u); }

// The block's rows of one array: pieces p = 0 .. rows * row_pieces - 1 of the contiguous destination range, lane t takes
// p = t, t + 256, ... and follows its (row, piece in row) with a PieceWalk (rows.h).
template <typename P>
__device__ __forceinline__ void move_array(const MoveArray& a, const int32_t* enc, int rows, int64_t first) {
  const uint32_t ppr = a.row_pieces;
  const uint32_t total = (uint32_t)rows * ppr;
  const bool copy_children = (a.flags & 1u) != 0;
  const P* __restrict__ src = reinterpret_cast<const P*>(a.src);
  P* __restrict__ dst = reinterpret_cast<P*>(a.dst) + first * (int64_t)ppr;
  PieceWalk w(threadIdx.x, ppr);
#pragma unroll 1
  for (uint32_t p = threadIdx.x; p < total; p += 256u * ROW_UNROLL) {
    P v[ROW_UNROLL];
#pragma unroll
    for (int u = 0; u < ROW_UNROLL; ++u) {
      v[u] = zero_piece<P>();
      if (p + 256u * u < total) {
        const int32_t e = enc[w.r];
        if (e >= 0 && (copy_children || !(e & CHILD_BIT)))
          v[u] = src[(int64_t)(e & (CHILD_BIT - 1)) * (int64_t)ppr + w.k];
      }
      w.advance();
    }
#pragma unroll
    for (int u = 0; u < ROW_UNROLL; ++u)
      if (p + 256u * u < total) dst[p + 256u * u] = v[u];
  }
}

__global__ void __launch_bounds__(256)
densify_move_kernel(MoveArgs m) {
  __shared__ int32_t enc[ROW_BLOCK];
  const int64_t first = (int64_t)blockIdx.x * ROW_BLOCK;
  const int64_t left = m.n_out - first;
  const int rows = left < ROW_BLOCK ? (int)left : ROW_BLOCK;
  {
    int32_t e = -1;
    if ((int)threadIdx.x < rows) {
      const int32_t s = m.src_row[first + threadIdx.x];
      if (s >= 0 && s < m.n_src) e = s | (m.child_slot[first + threadIdx.x] >= 0 ? CHILD_BIT : 0);
    }
    enc[threadIdx.x] = e;
  }
  __syncthreads();
#pragma unroll 1
  for (int gi = 0; gi < m.num_arrays; ++gi) {
    const MoveArray& a = m.a[gi];
    if (a.flags & 2u) move_array<uint4>(a, enc, rows, first);
    else move_array<uint32_t>(a, enc, rows, first);
  }
}

__device__ __forceinline__ float add_offset(float x, float off) { return off != 0.0f ? x + off : x; }
__device__ __forceinline__ float add_log_scale(float x, float scale) { return scale != 1.0f ? x + logf(scale) : x; }

// misc/renderer2d.py:36-43 (point_basis), :101-103 (repeat_sample_gaussians), :56-67 (split_with_offsets)
__global__ void __launch_bounds__(256)
densify_split2d_kernel(float* __restrict__ position, float* __restrict__ log_scaling, const float* __restrict__ rotation,
                       float* __restrict__ depths, int64_t first, int64_t count, int children,
                       const float* __restrict__ z, const float* __restrict__ scale, const float* __restrict__ depth_offset) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= count) return;
  const int64_t row = first + c, parent = c / children;
  const float rx = rotation[row * 2], ry = rotation[row * 2 + 1];
  const float norm = sqrtf(rx * rx + ry * ry);
  const float v1x = rx / norm, v1y = ry / norm;
  const float ls0 = log_scaling[row * 2], ls1 = log_scaling[row * 2 + 1];
  const float s0 = fmaxf(expf(ls0), 1e-4f), s1 = fmaxf(expf(ls1), 1e-4f);
  const float z0 = z[c * 2], z1 = z[c * 2 + 1];
  const float ox = (v1x * s0) * z0 + (-v1y * s1) * z1;
  const float oy = (v1y * s0) * z0 + (v1x * s1) * z1;
  position[row * 2] = add_offset(position[row * 2], ox);
  position[row * 2 + 1] = add_offset(position[row * 2 + 1], oy);
  if (scale) {
    log_scaling[row * 2] = add_log_scale(ls0, scale[parent * 2]);
    log_scaling[row * 2 + 1] = add_log_scale(ls1, scale[parent * 2 + 1]);
  }
  if (depths) {
    const float d = depths[row];
    depths[row] = fmaxf(depth_offset ? d + depth_offset[c] : d, 1e-6f);
  }
}

__global__ void __launch_bounds__(256)
densify_split3d_kernel(float* __restrict__ position, float* __restrict__ log_scaling, const float* __restrict__ rotation,
                       int64_t first, int64_t count, int children, const float* __restrict__ z,
                       const float* __restrict__ scale) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= count) return;
  const int64_t row = first + c, parent = c / children;
  float q[4], R[3][3], ls[3], sz[3];
  for (int k = 0; k < 4; ++k) q[k] = rotation[row * 4 + k];
  const float norm = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int k = 0; k < 4; ++k) q[k] = q[k] / norm;
  quat_to_mat(q, R);
  for (int k = 0; k < 3; ++k) {
    ls[k] = log_scaling[row * 3 + k];
    sz[k] = expf(ls[k]) * z[c * 3 + k];
  }
  for (int k = 0; k < 3; ++k) {
    const float off = R[k][0] * sz[0] + R[k][1] * sz[1] + R[k][2] * sz[2];
    position[row * 3 + k] = add_offset(position[row * 3 + k], off);
    if (scale) log_scaling[row * 3 + k] = add_log_scale(ls[k], scale[parent * 3 + k]);
  }
}

}  // namespace ms

using namespace ms;

static int check_plan_sizes(int64_t n, int children, const char* who) {
  if (n < 0) { set_error("%s: n >= 0 expected", who); return MS_ERR_BAD_ARG; }
  if (children < 1) { set_error("%s: children >= 1 expected (got %d)", who, children); return MS_ERR_BAD_ARG; }
  if (2 * n + 1 > INT32_MAX || n * (int64_t)children > INT32_MAX) {
    set_error("%s: row indexes must fit int32 (n = %lld, children = %d)", who, (long long)n, children);
    return MS_ERR_BAD_ARG;
  }
  return 0;
}

extern "C" int ms_densify_plan(const uint8_t* prune, const uint8_t* split, int64_t n, int children, int32_t* scan,
                               int32_t* counts, int32_t* counts_host, void* tmp, size_t* tmp_bytes, void* stream) {
  const int rc = check_plan_sizes(n, children, "ms_densify_plan");
  if (rc) return rc;
  MS_CHECK_TMP(tmp, tmp_bytes, scan_tmp_size(2 * n));       // the whole block is the scan's
  MS_CHECK_ARG(scan && counts, "null pointer");
  MS_CHECK_ARG(n == 0 || (prune && split), "null mask");
  hipStream_t s = (hipStream_t)stream;
  if (n > 0) {
    densify_flags_kernel<<<dim3((unsigned)div_up(n, 256)), dim3(256), 0, s>>>(prune, split, n, scan);
    MS_CHECK_LAUNCH();
  }
  const int rc2 = ms_exclusive_scan_i32(scan, 2 * n, scan, nullptr, tmp, tmp_bytes, stream);   // in place
  if (rc2) return rc2;
  densify_counts_kernel<<<dim3(1), dim3(64), 0, s>>>(scan, n, children, counts, counts_host);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_densify_table(const int32_t* scan, int64_t n, int children, int64_t n_out, int32_t* src_row,
                                int32_t* child_slot, void* stream) {
  const int rc = check_plan_sizes(n, children, "ms_densify_table");
  if (rc) return rc;
  MS_CHECK_ARG(n_out >= 0 && n_out <= n * (int64_t)children + n, "n_out out of range");
  if (n == 0 || n_out == 0) return 0;
  MS_CHECK_ARG(scan && src_row && child_slot, "null pointer");
  densify_table_kernel<<<dim3((unsigned)div_up(n, 256)), dim3(256), 0, (hipStream_t)stream>>>(scan, n, children, n_out,
                                                                                             src_row, child_slot);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_densify_move(const ms_densify_array* arrays, int num_arrays, const int32_t* src_row,
                               const int32_t* child_slot, int64_t n_src, int64_t n_out, void* stream) {
  MS_CHECK_ARG(num_arrays >= 0 && (arrays || num_arrays == 0), "bad array list");
  MS_CHECK_ARG(n_src >= 0 && n_src < CHILD_BIT, "0 <= n_src < 2^30 expected");
  MS_CHECK_ARG(n_out >= 0 && n_out <= INT32_MAX, "0 <= n_out < 2^31 expected");
  // every descriptor is checked before the first launch: an error return leaves every array as it was
  for (int i = 0; i < num_arrays; ++i) {
    const ms_densify_array& a = arrays[i];
    const int rc = check_row_array(__func__, i, a.struct_size, sizeof(ms_densify_array), a.row_bytes);
    if (rc) return rc;
    if (a.child_fill != 0 && a.child_fill != 1) { set_error("ms_densify_move: array %d: child_fill must be 0 (zero) or 1 (copy the parent)", i); return MS_ERR_BAD_ARG; }
    if (!a.src || !a.dst) { set_error("ms_densify_move: array %d: null pointer", i); return MS_ERR_BAD_ARG; }
    if (!aligned(4, {a.src, a.dst})) {
      set_error("ms_densify_move: array %d: bases must be 4-byte aligned", i);
      return MS_ERR_BAD_ARG;
    }
  }
  if (n_out == 0 || num_arrays == 0) return 0;
  MS_CHECK_ARG(src_row && child_slot, "null source table");
  MoveArgs m{};
  m.src_row = src_row; m.child_slot = child_slot; m.n_src = n_src; m.n_out = n_out;
  const dim3 grid((unsigned)div_up(n_out, ROW_BLOCK));
  for (int i = 0; i < num_arrays; ++i) {
    const ms_densify_array& a = arrays[i];
    const RowPieces pieces(a.row_bytes, {a.src, a.dst});
    MoveArray& out = m.a[m.num_arrays++];
    out.src = (const char*)a.src; out.dst = (char*)a.dst;
    out.row_pieces = pieces.row_pieces;
    out.flags = (a.child_fill ? 1u : 0u) | (pieces.vec ? 2u : 0u);
    if (m.num_arrays == ROW_MAX_ARRAYS || i == num_arrays - 1) {
      densify_move_kernel<<<grid, dim3(256), 0, (hipStream_t)stream>>>(m);
      MS_CHECK_LAUNCH();
      m.num_arrays = 0;
    }
  }
  return 0;
}

static int check_split(const void* position, const void* log_scaling, const void* rotation, int64_t first, int64_t count,
                       int children, const void* z, const char* who) {
  if (children < 1) { set_error("%s: children >= 1 expected (got %d)", who, children); return MS_ERR_BAD_ARG; }
  if (first < 0 || count < 0 || count % children != 0 || first + count > INT32_MAX) {
    set_error("%s: first >= 0 and count a non-negative multiple of children expected (first %lld, count %lld, children %d)",
              who, (long long)first, (long long)count, children);
    return MS_ERR_BAD_ARG;
  }
  if (count > 0 && !(position && log_scaling && rotation && z)) { set_error("%s: null pointer", who); return MS_ERR_BAD_ARG; }
  return 0;
}

extern "C" int ms_densify_split2d(float* position, float* log_scaling, const float* rotation, float* depths, int64_t first,
                                  int64_t count, int children, const float* z, const float* scale,
                                  const float* depth_offset, void* stream) {
  const int rc = check_split(position, log_scaling, rotation, first, count, children, z, "ms_densify_split2d");
  if (rc) return rc;
  MS_CHECK_ARG(depths || !depth_offset, "depth_offset without depths");
  if (count == 0) return 0;
  densify_split2d_kernel<<<dim3((unsigned)div_up(count, 256)), dim3(256), 0, (hipStream_t)stream>>>(
      position, log_scaling, rotation, depths, first, count, children, z, scale, depth_offset);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_densify_split3d(float* position, float* log_scaling, const float* rotation, int64_t first, int64_t count,
                                  int children, const float* z, const float* scale, void* stream) {
  const int rc = check_split(position, log_scaling, rotation, first, count, children, z, "ms_densify_split3d");
  if (rc) return rc;
  if (count == 0) return 0;
  densify_split3d_kernel<<<dim3((unsigned)div_up(count, 256)), dim3(256), 0, (hipStream_t)stream>>>(
      position, log_scaling, rotation, first, count, children, z, scale);
  MS_CHECK_LAUNCH();
  return 0;
}
