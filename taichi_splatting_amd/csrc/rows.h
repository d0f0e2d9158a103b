// rows.h — moving whole per-point rows as 16-byte or 4-byte pieces (included by common.h): the pieces, the division-free
// (row, piece in row) walk of a lane, the block-wide contiguous copies, and the host side of the two row movers
// (ms_densify_move, ms_relocate_move).  The constants and PieceWalk also compile with a plain host compiler
// (tests/test_rows_host.py walks PieceWalk against divmod); everything else needs hipcc, and the host side the
// set_error and aligned that common.h declares before it includes this file.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MS_ROWS_HD __host__ __device__ __forceinline__
#else
#define MS_ROWS_HD inline
#endif

namespace ms {

constexpr int ROW_BLOCK = 256;                 // rows per workgroup = lanes per workgroup
constexpr int ROW_UNROLL = 4;                  // pieces in flight per lane
constexpr int ROW_MAX_ARRAYS = 32;             // arrays per launch (a 3-D scene with Adam-like state has 17)
constexpr int64_t ROW_MAX_BYTES = 1 << 20;
// LDS table word of a row, written by the mover's kernel and read by its walk: source row | ROW_FLAG_BIT, or -1 (no
// source).  Source rows are below 2^30.
constexpr int32_t ROW_FLAG_BIT = 1 << 30;

// Where lane `lane` of a ROW_BLOCK-lane block stands in a run of rows of `row_pieces` pieces each, of which it takes
// pieces lane, lane + 256, ...: advance() moves 256 pieces on by (256 / row_pieces, 256 % row_pieces).  The piece step
// is below row_pieces and so is k, so k + step < 2 row_pieces: ONE carry, no division after the constructor.
struct PieceWalk {
  uint32_t r, k;                               // row of the run, piece in that row
  uint32_t row_pieces, step_r, step_k;
  MS_ROWS_HD PieceWalk(uint32_t lane, uint32_t pieces)
      : r(lane / pieces), k(lane % pieces), row_pieces(pieces), step_r(ROW_BLOCK / pieces), step_k(ROW_BLOCK % pieces) {}
  MS_ROWS_HD void advance() {
    r += step_r; k += step_k;
    if (k >= row_pieces) { k -= row_pieces; ++r; }
  }
};

#if defined(__HIPCC__)

typedef uint32_t __attribute__((may_alias)) piece4;
typedef uint32_t __attribute__((ext_vector_type(4), may_alias)) piece16;

template <typename P> __device__ __forceinline__ P zero_piece();
template <> __device__ __forceinline__ piece4 zero_piece<piece4>() { return 0u; }
template <> __device__ __forceinline__ piece16 zero_piece<piece16>() { return piece16{0u, 0u, 0u, 0u}; }

// total pieces of P from src to dst (which do not overlap), lane t of the block's ROW_BLOCK takes t, t + 256, ...; UNROLL
// loads are issued before the first store
template <int UNROLL, typename P>
__device__ __forceinline__ void copy_pieces(P* __restrict__ dst, const P* __restrict__ src, uint32_t total) {
  for (uint32_t p = threadIdx.x; p < total; p += ROW_BLOCK * UNROLL) {
    P v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
      if (p + ROW_BLOCK * u < total) v[u] = src[p + ROW_BLOCK * u];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
      if (p + ROW_BLOCK * u < total) dst[p + ROW_BLOCK * u] = v[u];
  }
}

// `bytes` (a multiple of 4) from src to dst, both 4-byte aligned; vec16: both 16-byte aligned
template <int UNROLL>
__device__ __forceinline__ void copy_range(void* dst, const void* src, uint32_t bytes, bool vec16) {
  if (vec16) {
    const uint32_t n16 = bytes >> 4;
    copy_pieces<UNROLL>(reinterpret_cast<piece16*>(dst), reinterpret_cast<const piece16*>(src), n16);
    copy_pieces<UNROLL>(reinterpret_cast<piece4*>(dst) + n16 * 4, reinterpret_cast<const piece4*>(src) + n16 * 4,
                        (bytes & 15u) >> 2);
  } else {
    copy_pieces<UNROLL>(reinterpret_cast<piece4*>(dst), reinterpret_cast<const piece4*>(src), bytes >> 2);
  }
}

// ---- host side of a row mover ------------------------------------------------------------------------------------------

// 16-byte pieces iff the row is a multiple of 16 bytes and every base is 16-byte aligned, else 4-byte pieces
struct RowPieces {
  uint32_t row_pieces;
  bool vec;
  RowPieces(int64_t row_bytes, std::initializer_list<const void*> bases)
      : vec(row_bytes % 16 == 0 && aligned(16, bases)) { row_pieces = (uint32_t)(row_bytes / (vec ? 16 : 4)); }
};

// the checks every row descriptor gets, whatever the mover: 0, MS_ERR_ABI or MS_ERR_BAD_ARG (with the error text set)
static inline int check_row_array(const char* who, int index, uint32_t struct_size, size_t expected_size, int64_t row_bytes) {
  if (struct_size != expected_size) {
    // "ms_densify_move" -> "ms_densify_array": the descriptor is named after its entry point
    const int stem = (int)(strrchr(who, '_') - who);
    set_error("%s: %.*s_array of another ABI (struct_size %u, this library: %u)", who, stem, who, struct_size, (unsigned)expected_size);
    return MS_ERR_ABI;
  }
  if (row_bytes <= 0 || row_bytes % 4 != 0 || row_bytes > ROW_MAX_BYTES) {
    set_error("%s: array %d: row_bytes must be a positive multiple of 4, at most %lld (got %lld)", who, index,
              (long long)ROW_MAX_BYTES, (long long)row_bytes);
    return MS_ERR_BAD_ARG;
  }
  return 0;
}

#endif  // __HIPCC__

}  // namespace ms
