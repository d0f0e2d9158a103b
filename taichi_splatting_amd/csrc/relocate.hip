// relocate.hip — fixed-budget densification (3DGS-MCMC, Kheradmand et al. 2024): N never changes.  Gaussians whose
// opacity has collapsed ("dead" rows) move onto live gaussians drawn in proportion to their opacity; every drawn
// gaussian and its copies get a corrected opacity and scale; after each optimiser step a covariance-shaped noise moves
// the positions (ms_perturb_positions).  No reference counterpart.  With torch this is a multinomial whose sample
// count is a host read, a bincount and one indexed copy per tensor and per state tensor; here nothing reads the host,
// nothing allocates and every array keeps its storage, so the whole step replays from a captured graph.
//
// Sequence (one stream, no host read):
//   weights  w_i = 0 for a dead row (!(alpha_logit > t), NaN included), else max(1, llrint(sigmoid(alpha_logit) 2^24))
//            evaluated in double, as int64; clears count[] and counts[] for the launches below.
//   cdf      inclusive int64 sum of the weights, made by the CALLER (torch.cumsum: exact on integers, so the draw does
//            not depend on the order a scan adds in; it is not the hot path).
//   draw     one lane per row: a dead row takes target = mulhi64(r_i, total) in [0, total), binary-searches the first j
//            with cdf[j] > target (always a live row), writes src[i] = j and adds 1 to count[j] (int32 atomic: an
//            integer, independent of order); a live row writes src[i] = i.  total == 0: every row keeps src[i] = i.
//   fresh    only rows with count > 0: ratio = min(count + 1, 51), o' = 1 - (1 - o)^(1 / ratio),
//            denom = sum_{i=1..ratio} sum_{k<i} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1), coeff = o / denom, in double from
//            the float32 inputs (in float32 the alternating sum is wrong by up to 3e-4), rounded once into the side
//            buffers fresh_opacity / fresh_scale.  The inner sum over i is an exact integer, C(ratio, k + 1) by the
//            hockey-stick identity = two neighbours of table row ratio - 1 (at most C(51, 26) < 2^53), so the loop
//            runs over k alone.
//   move     ONE launch for every array, in place: a workgroup takes 256 consecutive rows through all arrays.  The table
//            entry of a row is read once; a block with few touched rows compacts them into LDS (ballot prefix) and its
//            lanes walk the pieces of those rows alone, any other block walks all its rows; pieces are 16 bytes (row a
//            multiple of 16 bytes, bases 16-byte aligned) or 4 bytes.  An untouched row is neither read nor written.
// The hazard of working in place: a dead row reads its source's row while that source may be receiving its own new
// opacity and scale.  Sources are live and destinations dead, so copied arrays never overlap; opacity and scale reach
// BOTH the source and its copies from `fresh`, written by the earlier launch, never from the live array.
// HBM traffic of the move: per moved row and array row_bytes read + row_bytes written (zeroed rows: written only),
// + 8 bytes of table per row of the scene.
#include "common.h"

namespace ms {

constexpr int RELOC_COMPACT_BELOW = 8;     // a block with at most rows / 8 touched rows walks those alone
constexpr int32_t DRAWN_BIT = ROW_FLAG_BIT;     // LDS encoding of a row: -1 untouched | source row (moved) | own row + DRAWN_BIT
constexpr int MAX_RATIO = MS_RELOCATE_MAX_RATIO;

// Counting rows into one device word: a same-address atomic costs about 12 ns at the L2, so one per wave (94 K waves at
// 6 M rows) would take longer than the kernel's work.  The draw and fresh kernels therefore run a bounded grid with a
// grid-stride loop: a wave adds up the popcounts of its ballots (a scalar), the block adds its four waves in LDS and
// commits ONE atomic (block_count_commit, wave.h), at most COUNT_BLOCKS per launch.  Every lane of the block must
// reach both calls.
constexpr int COUNT_BLOCKS = 2048;

__global__ void __launch_bounds__(256)
relocate_weights_kernel(const float* __restrict__ alpha_logit, int64_t n, float threshold, int64_t* __restrict__ weights,
                        int32_t* __restrict__ count, int64_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 3) counts[i] = 0;
  if (i >= n) return;
  const float a = alpha_logit[i];
  int64_t w = 0;
  if (a > threshold) {
    w = llrint(16777216.0 / (1.0 + exp(-(double)a)));
    if (w < 1) w = 1;
  }
  weights[i] = w;
  count[i] = 0;
}

__global__ void __launch_bounds__(256)
relocate_draw_kernel(const int64_t* __restrict__ weights, const int64_t* __restrict__ cdf,
                     const uint64_t* __restrict__ random, int64_t n, int32_t* __restrict__ src, int32_t* count,
                     int64_t* counts) {
  const int64_t total = cdf[n - 1];
  uint32_t dead_rows = 0;
#pragma unroll 1
  for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    const bool in = i < n;
    const bool dead = in && weights[i] == 0;
    if (in) {
      int64_t s = i;
      if (dead && total > 0) {
        const uint64_t target = __umul64hi(random[i], (uint64_t)total);
        int64_t lo = 0, hi = n - 1;            // cdf[n - 1] = total > target: the answer is in [0, n - 1]
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if ((uint64_t)cdf[mid] > target) hi = mid;
          else lo = mid + 1;
        }
        s = lo;
        atomicAdd(count + lo, 1);
      }
      src[i] = (int32_t)s;
    }
    dead_rows += (uint32_t)__popcll(__ballot(dead));
  }
  block_count_commit(dead_rows, counts);
  if (blockIdx.x == 0 && threadIdx.x == 0) counts[2] = total;
}

__global__ void __launch_bounds__(256)
relocate_fresh_kernel(const float* __restrict__ alpha_logit, const float* __restrict__ log_scaling, int dims,
                      const int32_t* __restrict__ count, int64_t n, double min_opacity, const double* __restrict__ binom,
                      float* __restrict__ fresh_opacity, float* __restrict__ fresh_scale, int64_t* counts) {
  uint32_t drawn_rows = 0;
#pragma unroll 1
  for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    const int32_t c = i < n ? count[i] : 0;
    const bool drawn = c > 0;
    if (drawn) {
      const int ratio = c + 1 < MAX_RATIO ? c + 1 : MAX_RATIO;
      const double o = 1.0 / (1.0 + exp(-(double)alpha_logit[i]));
      const double on = 1.0 - pow(1.0 - o, 1.0 / (double)ratio);
      const double* __restrict__ row = binom + (ratio - 1) * MAX_RATIO;
      double denom = 0.0, p = 1.0;
#pragma unroll 1
      for (int k = 0; k < ratio; ++k) {
        p *= on;
        // sum_{i = k + 1 .. ratio} C(i - 1, k) = C(ratio, k + 1) = C(ratio - 1, k) + C(ratio - 1, k + 1): exact integers
        const double column = row[k] + (k + 1 < MAX_RATIO ? row[k + 1] : 0.0);
        const double term = p / sqrt((double)(k + 1)) * column;
        denom += (k & 1) ? -term : term;
      }
      const double ln_coeff = log(o / denom);
      const double oc = fmin(fmax(on, min_opacity), 1.0 - 1e-7);
      fresh_opacity[i] = (float)log(oc / (1.0 - oc));
      for (int d = 0; d < dims; ++d) fresh_scale[i * dims + d] = (float)((double)log_scaling[i * dims + d] + ln_coeff);
    }
    drawn_rows += (uint32_t)__popcll(__ballot(drawn));
  }
  block_count_commit(drawn_rows, counts + 1);
}

struct RelocArray {
  char* data;
  const char* fresh;
  uint32_t row_pieces;               // pieces (of 16 or 4 bytes) per row
  uint32_t flags;                    // bits 0-1: ACTION_*, bit 2: 16-byte pieces
};
enum { ACTION_COPY = 0, ACTION_ZERO = 1, ACTION_FRESH = 2 };

struct RelocArgs {
  const int32_t* src;
  const int32_t* count;
  int64_t n;
  int num_arrays;
  RelocArray a[ROW_MAX_ARRAYS];
};

// The listed rows of the block in one array: pieces p = 0 .. listed * row_pieces - 1, lane t takes p = t, t + 256, ... and
// follows its (touched row, piece in row) with a PieceWalk (rows.h).  Consecutive lanes take consecutive pieces of a row, and consecutive touched rows where rows are short.  All loads of a
// round are issued before its first store.  Reads come from live rows (or `fresh`), writes go to dead rows or to the
// lane's own row: no lane reads what another writes.
template <typename P>
__device__ __forceinline__ void relocate_array(const RelocArray& a, const int32_t* enc, const uint8_t* row_of, int touched,
                                               int64_t first) {
  const uint32_t ppr = a.row_pieces;
  const uint32_t total = (uint32_t)touched * ppr;
  const uint32_t action = a.flags & 3u;
  const P* from = reinterpret_cast<const P*>(action == ACTION_FRESH ? a.fresh : a.data);
  P* dst = reinterpret_cast<P*>(a.data) + first * (int64_t)ppr;
  PieceWalk w(threadIdx.x, ppr);
#pragma unroll 1
  for (uint32_t p = threadIdx.x; p < total; p += 256u * ROW_UNROLL) {
    P v[ROW_UNROLL];
    uint32_t at[ROW_UNROLL];
    bool write[ROW_UNROLL];
#pragma unroll
    for (int u = 0; u < ROW_UNROLL; ++u) {
      v[u] = zero_piece<P>();
      write[u] = false;
      at[u] = 0;
      if (p + 256u * u < total) {
        const int32_t e = enc[w.r];
        if (e >= 0 && (action != ACTION_COPY || !(e & DRAWN_BIT))) {
          write[u] = true;
          at[u] = (uint32_t)row_of[w.r] * ppr + w.k;
          if (action != ACTION_ZERO) v[u] = from[(int64_t)(e & (DRAWN_BIT - 1)) * (int64_t)ppr + w.k];
        }
      }
      w.advance();
    }
#pragma unroll
    for (int u = 0; u < ROW_UNROLL; ++u)
      if (write[u]) dst[at[u]] = v[u];
  }
}

__global__ void __launch_bounds__(256)
relocate_move_kernel(RelocArgs m) {
  __shared__ int32_t enc[ROW_BLOCK];         // the rows to walk (the touched ones in row order, or all): source | DRAWN_BIT, -1
  __shared__ uint8_t row_of[ROW_BLOCK];      // ... and their row within the block
  __shared__ int wave_touched[4];
  const int64_t first = (int64_t)blockIdx.x * ROW_BLOCK;
  const int64_t left = m.n - first;
  const int rows = left < ROW_BLOCK ? (int)left : ROW_BLOCK;
  int32_t e = -1;
  if ((int)threadIdx.x < rows) {
    const int64_t row = first + threadIdx.x;
    const int32_t s = m.src[row];
    if (s != row) { if (s >= 0 && s < m.n) e = s; }              // a dead row that moves onto row s
    else if (m.count[row] > 0) e = (int32_t)row | DRAWN_BIT;     // a live row that was drawn
  }
  const unsigned long long mask = __ballot(e >= 0);
  const int wave = (int)(threadIdx.x >> 6);
  if (lane_id() == 0) wave_touched[wave] = __popcll(mask);
  __syncthreads();
  int before = 0, touched = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wave) before += wave_touched[w];
    touched += wave_touched[w];
  }
  if (touched == 0) return;
  // Few touched rows: walk those alone.  Many: walk every row of the block, whose stores then cover whole runs of
  // neighbouring rows (measured at 6 M rows x 716 bytes: 2 % touched 0.17 ms compacted against 0.34 ms, 19 % touched
  // 0.60 against 0.53, 80 % touched 1.53 against 1.22).
  const bool compact = touched * RELOC_COMPACT_BELOW <= rows;
  if (!compact) {
    enc[threadIdx.x] = e;
    row_of[threadIdx.x] = (uint8_t)threadIdx.x;
    touched = rows;
  } else if (e >= 0) {
    const int at = before + lane_rank_popc(mask);
    enc[at] = e;
    row_of[at] = (uint8_t)threadIdx.x;
  }
  __syncthreads();
#pragma unroll 1
  for (int gi = 0; gi < m.num_arrays; ++gi) {
    const RelocArray& a = m.a[gi];
    if (a.flags & 4u) relocate_array<piece16>(a, enc, row_of, touched, first);
    else relocate_array<piece4>(a, enc, row_of, touched, first);
  }
}

// ---- position noise ------------------------------------------------------------------------------------------------
// One lane per gaussian, a workgroup takes 256 consecutive rows.  The three 12-byte-per-row arrays (position,
// log_scaling, z) are contiguous over the block: they move between HBM and LDS as 16-byte pieces (4-byte pieces when a
// base is not 16-byte aligned, and for the tail of a partial last block), each lane then reads its row from LDS (stride
// of 3 words: no bank conflicts).  rotation is one 16-byte load per lane, alpha_logit one coalesced word.
// 56 bytes per row in, 12 out.

__device__ __forceinline__ float add_nonzero(float x, float off) { return off != 0.0f ? x + off : x; }

__global__ void __launch_bounds__(ROW_BLOCK)
perturb_positions_kernel(float* position, const float* __restrict__ log_scaling, const float* __restrict__ rotation,
                         const float* __restrict__ alpha_logit, const float* __restrict__ z, int64_t n, float step,
                         double k, double x0, int vec16) {
  __shared__ __attribute__((aligned(16))) float lds_p[ROW_BLOCK * 3];
  __shared__ __attribute__((aligned(16))) float lds_s[ROW_BLOCK * 3];
  __shared__ __attribute__((aligned(16))) float lds_z[ROW_BLOCK * 3];
  const int64_t first = (int64_t)blockIdx.x * ROW_BLOCK;
  const int64_t left = n - first;
  const int rows = left < ROW_BLOCK ? (int)left : ROW_BLOCK;
  const uint32_t bytes = (uint32_t)rows * 12u;
  copy_range<1>(lds_p, position + first * 3, bytes, vec16 != 0);
  copy_range<1>(lds_s, log_scaling + first * 3, bytes, vec16 != 0);
  copy_range<1>(lds_z, z + first * 3, bytes, vec16 != 0);
  __syncthreads();
  const int t = (int)threadIdx.x;
  if (t < rows) {
    const int64_t row = first + t;
    // step g(o), g(o) = 1 / (1 + exp(-k ((1 - o) - x0))), in double: k = 100 turns one float32 rounding of 1 - o into
    // 6e-6 of g, and for an opaque gaussian g is far below the float32 normal range (e^-99.5) while the offset need not be
    const double o = 1.0 / (1.0 + exp(-(double)alpha_logit[row]));
    const double factor = (double)step / (1.0 + exp(-k * ((1.0 - o) - x0)));
    float q[4];
    if (vec16) {
      const float4 q4 = *reinterpret_cast<const float4*>(rotation + row * 4);
      q[0] = q4.x; q[1] = q4.y; q[2] = q4.z; q[3] = q4.w;
    } else {
      for (int j = 0; j < 4; ++j) q[j] = rotation[row * 4 + j];
    }
    const float qn = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    // a zero or non-finite quaternion has no covariance (the projection culls such a row): the row stays
    if (factor != 0.0 && qn > 0.0f && qn <= 3.4028234664e38f) {
      float R[3][3], y[3];
      for (int j = 0; j < 4; ++j) q[j] = q[j] / qn;
      quat_to_mat(q, R);
      const float z0 = lds_z[t * 3], z1 = lds_z[t * 3 + 1], z2 = lds_z[t * 3 + 2];
      for (int j = 0; j < 3; ++j)            // diag(exp(2 log_scaling)) R^T z
        y[j] = (R[0][j] * z0 + R[1][j] * z1 + R[2][j] * z2) * expf(2.0f * lds_s[t * 3 + j]);
      for (int j = 0; j < 3; ++j) {
        const float v = R[j][0] * y[0] + R[j][1] * y[1] + R[j][2] * y[2];
        lds_p[t * 3 + j] = add_nonzero(lds_p[t * 3 + j], (float)(factor * (double)v));      // rounded once
      }
    }
  }
  __syncthreads();
  copy_range<1>(position + first * 3, lds_p, bytes, vec16 != 0);
}

}  // namespace ms

using namespace ms;

static int64_t count_grid(int64_t n) { const int64_t b = div_up(n, 256); return b < COUNT_BLOCKS ? b : COUNT_BLOCKS; }

static int check_rows(int64_t n, const char* who) {
  if (n < 0 || n >= DRAWN_BIT) { set_error("%s: 0 <= n < 2^30 expected (got %lld)", who, (long long)n); return MS_ERR_BAD_ARG; }
  return 0;
}

extern "C" int ms_relocate_weights(const float* alpha_logit, int64_t n, float threshold, int64_t* weights, int32_t* count,
                                   int64_t* counts, void* stream) {
  const int rc = check_rows(n, "ms_relocate_weights");
  if (rc) return rc;
  MS_CHECK_ARG(counts != nullptr && aligned(8, {counts}), "counts: 3 int64 expected");
  MS_CHECK_ARG(n == 0 || (alpha_logit && weights && count), "null pointer");
  MS_CHECK_ARG(aligned(4, {alpha_logit, count}) && aligned(8, {weights}), "misaligned pointer");
  MS_CHECK_ARG(!(threshold != threshold), "threshold is NaN");
  relocate_weights_kernel<<<dim3((unsigned)div_up(n > 3 ? n : 3, 256)), dim3(256), 0, (hipStream_t)stream>>>(
      alpha_logit, n, threshold, weights, count, counts);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_relocate_draw(const int64_t* weights, const int64_t* cdf, const uint64_t* random, int64_t n,
                                int32_t* src, int32_t* count, int64_t* counts, void* stream) {
  const int rc = check_rows(n, "ms_relocate_draw");
  if (rc) return rc;
  if (n == 0) return 0;
  MS_CHECK_ARG(weights && cdf && random && src && count && counts, "null pointer");
  MS_CHECK_ARG(aligned(8, {weights, cdf, random, counts}) && aligned(4, {src, count}), "misaligned pointer");
  relocate_draw_kernel<<<dim3((unsigned)count_grid(n)), dim3(256), 0, (hipStream_t)stream>>>(weights, cdf, random, n, src,
                                                                                             count, counts);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_relocate_fresh(const float* alpha_logit, const float* log_scaling, int scale_dims, const int32_t* count,
                                 int64_t n, double min_opacity, const double* binomials, float* fresh_opacity,
                                 float* fresh_scale, int64_t* counts, void* stream) {
  const int rc = check_rows(n, "ms_relocate_fresh");
  if (rc) return rc;
  MS_CHECK_ARG(scale_dims >= 1 && scale_dims <= 16, "1 <= scale_dims <= 16 expected");
  MS_CHECK_ARG(min_opacity > 0.0 && min_opacity < 1.0 - 1e-7, "0 < min_opacity < 1 - 1e-7 expected");
  if (n == 0) return 0;
  MS_CHECK_ARG(alpha_logit && log_scaling && count && binomials && fresh_opacity && fresh_scale && counts, "null pointer");
  MS_CHECK_ARG(aligned(4, {alpha_logit, log_scaling, count, fresh_opacity, fresh_scale}) && aligned(8, {binomials, counts}),
               "misaligned pointer");
  relocate_fresh_kernel<<<dim3((unsigned)count_grid(n)), dim3(256), 0, (hipStream_t)stream>>>(
      alpha_logit, log_scaling, scale_dims, count, n, min_opacity, binomials, fresh_opacity, fresh_scale, counts);
  MS_CHECK_LAUNCH();
  return 0;
}

extern "C" int ms_relocate_move(const ms_relocate_array* arrays, int num_arrays, const int32_t* src, const int32_t* count,
                                int64_t n, void* stream) {
  const int rc = check_rows(n, "ms_relocate_move");
  if (rc) return rc;
  MS_CHECK_ARG(num_arrays >= 0 && (arrays || num_arrays == 0), "bad array list");
  // every descriptor is checked before the first launch: an error return leaves every array as it was
  for (int i = 0; i < num_arrays; ++i) {
    const ms_relocate_array& a = arrays[i];
    const int rc_row = check_row_array(__func__, i, a.struct_size, sizeof(ms_relocate_array), a.row_bytes);
    if (rc_row) return rc_row;
    if (a.role < MS_RELOCATE_COPY || a.role > MS_RELOCATE_SCALE) {
      set_error("ms_relocate_move: array %d: unknown role %d", i, a.role);
      return MS_ERR_BAD_ARG;
    }
    const bool wants_fresh = a.role == MS_RELOCATE_OPACITY || a.role == MS_RELOCATE_SCALE;
    if (!a.data || (wants_fresh && !a.fresh)) { set_error("ms_relocate_move: array %d: null pointer", i); return MS_ERR_BAD_ARG; }
    if (!aligned(4, {a.data, wants_fresh ? a.fresh : nullptr})) {
      set_error("ms_relocate_move: array %d: bases must be 4-byte aligned", i);
      return MS_ERR_BAD_ARG;
    }
    if (wants_fresh && a.fresh == a.data) {
      set_error("ms_relocate_move: array %d: fresh must be a side buffer, not the array itself", i);
      return MS_ERR_BAD_ARG;
    }
  }
  if (n == 0 || num_arrays == 0) return 0;
  MS_CHECK_ARG(src && count, "null source table");
  RelocArgs m{};
  m.src = src; m.count = count; m.n = n;
  const dim3 grid((unsigned)div_up(n, ROW_BLOCK));
  for (int i = 0; i < num_arrays; ++i) {
    const ms_relocate_array& a = arrays[i];
    const bool wants_fresh = a.role == MS_RELOCATE_OPACITY || a.role == MS_RELOCATE_SCALE;
    RelocArray& out = m.a[m.num_arrays++];
    out.data = (char*)a.data;
    out.fresh = wants_fresh ? (const char*)a.fresh : nullptr;
    const RowPieces pieces(a.row_bytes, {out.data, out.fresh});
    out.row_pieces = pieces.row_pieces;
    out.flags = (wants_fresh ? ACTION_FRESH : a.role == MS_RELOCATE_ZERO_TOUCHED ? ACTION_ZERO : ACTION_COPY) | (pieces.vec ? 4u : 0u);
    if (m.num_arrays == ROW_MAX_ARRAYS || i == num_arrays - 1) {
      relocate_move_kernel<<<grid, dim3(256), 0, (hipStream_t)stream>>>(m);
      MS_CHECK_LAUNCH();
      m.num_arrays = 0;
    }
  }
  return 0;
}

extern "C" int ms_perturb_positions(float* position, const float* log_scaling, const float* rotation,
                                    const float* alpha_logit, const float* z, int64_t n, float step, double k, double x0,
                                    void* stream) {
  MS_CHECK_ARG(n >= 0 && n <= INT32_MAX, "0 <= n < 2^31 expected");
  MS_CHECK_ARG(step == step && k == k && x0 == x0, "step, k and x0 must not be NaN");
  if (n == 0) return 0;
  MS_CHECK_ARG(position && log_scaling && rotation && alpha_logit && z, "null pointer");
  MS_CHECK_ARG(aligned(4, {position, log_scaling, rotation, alpha_logit, z}), "misaligned pointer");
  const int vec16 = aligned(16, {position, log_scaling, rotation, z});
  perturb_positions_kernel<<<dim3((unsigned)div_up(n, ROW_BLOCK)), dim3(ROW_BLOCK), 0, (hipStream_t)stream>>>(
      position, log_scaling, rotation, alpha_logit, z, n, step, k, x0, vec16);
  MS_CHECK_LAUNCH();
  return 0;
}
