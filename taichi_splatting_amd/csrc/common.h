// common.h — shared host/device helpers for the gfx950 kernels (wave64 only): error reporting, scratch blocks, splat
// rows, the depth sort key.  The wave and block primitives (lane_id, DPP moves, butterflies, scans, ballot ranks,
// one-atomic-per-block commits) live in wave.h, the row pieces and the walk of the row movers in rows.h; this header
// includes both.
#pragma once

#include <hip/hip_runtime.h>
#include <initializer_list>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/mi355_splat.h"
#include "splat_math.h"
#include "wave.h"

namespace ms {

// ---- error reporting ---------------------------------------------------------------------------
void set_error(const char* fmt, ...);

#define MS_CHECK_ARG(cond, msg)                                  \
  do {                                                           \
    if (!(cond)) {                                               \
      ms::set_error("%s: %s", __func__, msg);                    \
      return MS_ERR_BAD_ARG;                                     \
    }                                                            \
  } while (0)

#define MS_CHECK_LAUNCH()                                                         \
  do {                                                                            \
    hipError_t e__ = hipGetLastError();                                           \
    if (e__ != hipSuccess) {                                                      \
      ms::set_error("%s: kernel launch failed: %s", __func__, hipGetErrorString(e__)); \
      return (int)e__;                                                            \
    }                                                                             \
  } while (0)

#define MS_CHECK_HIP(expr)                                                        \
  do {                                                                            \
    hipError_t e__ = (expr);                                                      \
    if (e__ != hipSuccess) {                                                      \
      ms::set_error("%s: %s failed: %s", __func__, #expr, hipGetErrorString(e__)); \
      return (int)e__;                                                            \
    }                                                                             \
  } while (0)

static inline int64_t div_up(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t a, size_t b) { return (a + b - 1) / b * b; }

// every pointer is a multiple of `bytes` (a power of two); a null pointer counts as aligned
static inline bool aligned(uintptr_t bytes, std::initializer_list<const void*> pointers) {
  uintptr_t bits = 0;
  for (const void* p : pointers) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & (bytes - 1)) == 0;
}

}  // namespace ms

#include "rows.h"      // after set_error and aligned, which its host side uses

namespace ms {

// ---- scratch blocks: the (tmp, tmp_bytes) convention of include/mi355_splat.h ------------------------------------
// Every entry point with a scratch block lays it out with ONE Carve and answers the two-call protocol with ONE
// MS_CHECK_TMP, after its shape checks and before its null-pointer checks; nothing else sizes or splits a block.
// The carver: a running offset in units of 256 bytes.  An empty region takes no room (and shares its offset with the
// next one); a layout that gives empty regions a place of their own passes max(bytes, 1).
struct Carve {
  size_t off = 0;       // bytes taken so far: the size of the block once every region is taken
  size_t take(size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; }
  static size_t one(size_t bytes) { return align_up(bytes, 256); }   // size of a block with a single region (at offset 0)
};
template <class T>
static inline T* at(void* base, size_t off) { return (T*)((char*)base + off); }

// scratch of the scan and the radix sort (scan_sort.hip), for the stages that nest them in their own block
size_t scan_tmp_size(int64_t n);
size_t sort_tmp_size(int64_t n, int key_bytes, bool adaptive = false);   // adaptive: depth_argsort_launch's layout

// true: the entry point returns *rc now (null tmp_bytes, a size query answered, or a block that is too small)
static inline bool tmp_answered(const char* who, const void* tmp, size_t* tmp_bytes, size_t need, int too_small, int* rc) {
  if (tmp_bytes == nullptr) { set_error("%s: tmp_bytes is null", who); *rc = MS_ERR_BAD_ARG; return true; }
  if (tmp == nullptr) { *tmp_bytes = need; *rc = 0; return true; }
  if (*tmp_bytes < need) {
    set_error("%s: tmp_bytes too small (%zu < %zu)", who, *tmp_bytes, need);
    *rc = too_small;
    return true;
  }
  return false;
}
#define MS_CHECK_TMP_AS(tmp, tmp_bytes, need, too_small)                                   \
  do {                                                                                     \
    int rc__;                                                                              \
    if (ms::tmp_answered(__func__, tmp, tmp_bytes, need, too_small, &rc__)) return rc__;   \
  } while (0)
#define MS_CHECK_TMP(tmp, tmp_bytes, need) MS_CHECK_TMP_AS(tmp, tmp_bytes, need, MS_ERR_TMP_TOO_SMALL)

// Splat rows (round 5): ONE 64-byte row per gaussian — [points7 (0..6) | depth (7) | colour (8..10) | unused] — from
// which the product raster kernels gather a splat with three 16-byte loads out of ONE 128-byte line instead of ten
// 4-byte loads out of two or three lines (28- and 12-byte rows straddle): config D at tile 16, same box, backward
// 1.331 -> 1.249 ms, forward 0.626 -> 0.596 ms (tools/rbench.py --rows; 48-byte rows: 1.266 / 0.604; the two arrays
// merely padded to 32- and 16-byte rows: 1.305 / 0.630 — it is the line count, not the load width).  Offered through
// the C-ABI (ms_splat_rows_pack, ms_raster_fwd_rows, ms_raster_bwd_moments_rows); the frame executor can fill such a
// table in its projection and SH kernels but does not by default: see frame.hip, frame_uses_rows.
constexpr int SPLAT_ROW = 16;
constexpr int SPLAT_ROW_COLOUR = 8;

// 32 bit sort key of the depth pre-sort: float bits (non-negative depths keep their order) or the 16 bit quantisation
// of make_sort_key (tile_mapper.py:55-61).  near_plane > 0 fuses ndc_depth (torch_lib/projection.py:120-123,
// renderer.py:67): evaluated in double from the depth's own precision, then rounded once to the float the key is made of.
template <typename T>
__device__ __forceinline__ uint32_t depth_sort_key(T depth, int depth16, double near_plane, double far_plane) {
  float d;
  if (near_plane > 0.0) {
    const double dd = (double)depth;
    d = (float)(1.0 - (1.0 / dd - 1.0 / far_plane) / (1.0 / near_plane - 1.0 / far_plane));
  } else {
    d = (float)depth;
  }
  return depth16 ? (uint32_t)(fminf(fmaxf(d, 0.0f), 1.0f) * 65535.0f) : __float_as_uint(d);
}

}  // namespace ms
