/* mi355_splat.h — C-ABI of libmi355_splat.so: the gfx950 (MI355X) back end of the
 * taichi_splatting render path (projection -> SH colour -> tile mapper -> alpha composite).
 *
 * Conventions
 *   - every function returns 0 on success, a positive hipError_t on a HIP failure or a negative
 *     MS_ERR_* code on an argument error; ms_last_error_string() describes the last failure.
 *   - all pointers are DEVICE pointers unless the name ends in _host; tensors are contiguous,
 *     row-major; image_size is (W, H), images are (H, W, C).
 *   - no function allocates device memory or synchronises: callers own every buffer, scratch included.
 *   - scratch blocks, (tmp, tmp_bytes) — one convention for every function with that pair (ms_map_tiles_direct names
 *     it (scratch, scratch_bytes)): called with tmp == NULL the function stores the size the block must have for these
 *     sizes in *tmp_bytes, returns 0 and does nothing else — data pointers may be NULL, no stream is touched.  The size
 *     is a multiple of 256 bytes, depends on the size arguments alone, and may be 0.  Called with a block, *tmp_bytes is
 *     the block's size (read, never written) and the function carves its arrays from the block at offsets that are
 *     multiples of 256 bytes: a block aligned to 256 bytes gives every array that alignment (the ms_mesh_* functions
 *     require it of tmp and return MS_ERR_BAD_ARG otherwise; ms_map_tiles_direct requires 16 bytes; the rest take any
 *     address hipMalloc or a tensor allocator returns).  Errors, checked after the size arguments and before the data
 *     pointers: tmp_bytes == NULL is MS_ERR_BAD_ARG; a block smaller than the reported size is MS_ERR_TMP_TOO_SMALL
 *     with the message "<function>: tmp_bytes too small (<given> < <needed>)", and nothing is launched.  One exception,
 *     kept for its callers: ms_knn_points returns MS_ERR_BAD_ARG, with the same message, for a block that is too small.
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream).
 *   - dtype selects the float (MS_F32) or double (MS_F64) instantiation, the way the reference
 *     specialises its Taichi kernels on the tensor dtype (rasterizer/function.py:126).
 *
 * Each entry point names the reference interface it replaces (paths relative to
 * /root/reference/taichi_splatting).
 */
#ifndef MI355_SPLAT_H
#define MI355_SPLAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 0.5.0 (round 6).  The hundreds digit is the ABI generation: it changes whenever a struct below changes layout or a
 * function changes its signature.  500: ms_frame_desc / ms_frame_inputs / ms_frame_grads start with their own size (and
 * ms_frame_desc with the caller's MS_VERSION) — every ms_frame_* call rejects a struct of another size or generation
 * with MS_ERR_ABI instead of reading fields that are not where it expects them (round 5 grew ms_frame_desc and
 * ms_frame_layout under version 400); split_min_run / split_seg_len parameters of the ms_raster_*_split functions,
 * ms_frame_desc.split_seg_len; ms_optim_* (fused optimiser groups).
 * 501 (0.5.1): the direct-order mapper has one construction — the two entry points of the u64-key form (emission of
 * tile << 32 | depth key with int32 values, per-tile sort of such keys) are gone, ms_tile_payload_sort is the per-tile
 * sort on its own.  No struct changed: the generation stays 5 and sized structs built against 500 are accepted. */
#define MS_VERSION 501
#define MS_ABI_GENERATION(version) ((version) / 100)

enum { MS_F32 = 0, MS_F64 = 1 };

enum {
  MS_ERR_BAD_ARG = -1,      /* null pointer / negative size / unsupported enum */
  MS_ERR_UNSUPPORTED = -2,  /* valid request with no compiled instantiation (e.g. F > 4) */
  MS_ERR_TMP_TOO_SMALL = -3,
  MS_ERR_ABI = -4           /* a struct's leading struct_size / abi_version is not this library's */
};

/* Compile-time constants of the reference's RasterConfig (data_types.py:17-47) that the raster
 * kernels consume at run time. */
typedef struct ms_raster_config {
  int32_t tile_size;               /* 8, 16 or 32 */
  int32_t antialias;               /* gaussian_pdf_antialias instead of gaussian_pdf */
  int32_t use_alpha_blending;      /* 0: quantile ("median") render, forward only */
  int32_t compute_visibility;
  int32_t compute_point_heuristic;
  int32_t reserved;
  double clamp_max_alpha;
  double alpha_threshold;
  double saturate_threshold;
} ms_raster_config;

int ms_version(void);
const char* ms_last_error_string(void);

/* ---- perspective projection ------------------------------------------------------------------
 * ms_project_fwd replaces project_kernel (perspective/projection.py:33-81): per gaussian, packed
 * 2D gaussian [mean2, axis2, sigma2, alpha] into out_points7[i], camera depth into out_depth[i]
 * (0 when culled) and the in-view flag (0/1) into out_flag[i].  T_camera_world is the (4,4)
 * row-major matrix (rows 0..2 used), projection = [fx, fy, cx, cy]; both are device pointers so
 * that no host read-back of camera tensors is needed (the reference replicates them per point,
 * projection.py:215-216). */
int ms_project_fwd(const void* position, const void* log_scaling, const void* rotation,
                   const void* alpha_logit, const void* T_camera_world, const void* projection,
                   int image_w, int image_h, double near_plane, double far_plane,
                   double blur_cov, double clamp_margin, double alpha_threshold,
                   int64_t n, void* out_points7, void* out_depth, int32_t* out_flag,
                   int dtype, void* stream);

/* Compaction replacing torch.nonzero + 2 gathers (projection.py:147-150).  scan = exclusive scan
 * of the flags (n+1 entries, ms_exclusive_scan_i32).  Writes the V visible rows: out_points7
 * (V,7), out_depth (V), optional out_ndc_depth (V) = 1-(1/d-1/far)/(1/near-1/far)
 * (torch_lib/projection.py:120-123, fused) and out_indexes (V) int64. */
int ms_project_gather(const void* points7, const void* depth, const int32_t* flag,
                      const int32_t* scan, int64_t n, double near_plane, double far_plane,
                      void* out_points7, void* out_depth, void* out_ndc_depth,
                      int64_t* out_indexes, int dtype, void* stream);

/* ms_project_bwd replaces indexed_project_kernel.grad (projection.py:85-119,167-188): hand-derived
 * reverse mode.  Rows indexes[i] of the N-sized outputs are WRITTEN (rows of culled gaussians are
 * left untouched: pre-zero them); grad_camera (16 values: dT[3][4] row-major then d[fx,fy,cx,cy])
 * is ACCUMULATED atomically and may be NULL; grad_depth may be NULL (no gradient reaches the depth output). */
int ms_project_bwd(const void* position, const void* log_scaling, const void* rotation,
                   const void* alpha_logit, const void* T_camera_world, const void* projection,
                   int image_w, int image_h, double blur_cov, double clamp_margin,
                   const int64_t* indexes, int64_t v, const void* grad_points7,
                   const void* grad_depth, void* grad_position, void* grad_log_scaling,
                   void* grad_rotation, void* grad_alpha_logit, void* grad_camera,
                   int dtype, void* stream);

/* ---- spherical harmonics ---------------------------------------------------------------------
 * evaluate_sh_at_kernel (indexed_spherical_harmonics.py:119-134): out[i,c] =
 * clamp(sum_d Y_d(normalise(pos[idx]-cam)) * params[idx,c,d] + 0.5, 0, 1); params is (M, F, D),
 * D = (degree+1)^2, degree in [0,3]. */
int ms_sh_fwd(const void* params, const void* positions, const int64_t* indexes,
              const void* camera_pos, int64_t v, int f, int degree, void* out,
              int dtype, void* stream);

/* ms_sh_fwd at an ACTIVE degree (the SH band schedule of a trainer, a diffuse-only view): params is stored at `degree`,
 * (M, F, (degree+1)^2), and only its first (active_degree+1)^2 coefficients per channel are evaluated, in place — the
 * colours of the sliced tensor params[:, :, :(active_degree+1)^2].  0 <= active_degree <= degree;
 * ms_sh_fwd(.., degree, ..) is ms_sh_fwd_active(.., degree, degree, ..). */
int ms_sh_fwd_active(const void* params, const void* positions, const int64_t* indexes,
                     const void* camera_pos, int64_t v, int f, int degree, int active_degree, void* out,
                     int dtype, void* stream);

/* evaluate_sh_at_kernel.grad (indexed_spherical_harmonics.py:153-160).  grad_params (M,F,D),
 * grad_positions (M,3) and grad_camera_pos (3) are ACCUMULATED atomically (indexes may repeat);
 * any of them may be NULL.  out = the saved forward output (V,F) or NULL: with it, and when only
 * grad_params is requested (the renderer detaches positions, renderer.py:53), a streaming kernel
 * with coalesced row writes is used; unique_indexes != 0 additionally promises that indexes holds
 * no repeats (true for the projection's compaction list), so rows are WRITTEN with plain stores
 * (rows not listed stay untouched: pre-zero grad_params). */
int ms_sh_bwd(const void* params, const void* positions, const int64_t* indexes,
              const void* camera_pos, int64_t v, int f, int degree, const void* out,
              const void* grad_out, void* grad_params, void* grad_positions,
              void* grad_camera_pos, int unique_indexes, int dtype, void* stream);

/* ms_sh_bwd at an active degree: grad_params keeps the stored shape (M, F, (degree+1)^2); the gradient of the inactive
 * coefficients is exactly zero — written as zeros wherever whole rows are written (`out` given, f <= 4,
 * unique_indexes), left at the caller's zeros where rows are accumulated — and grad_positions / grad_camera_pos see
 * the active bands only.  ms_sh_bwd(.., degree, ..) is ms_sh_bwd_active(.., degree, degree, ..). */
int ms_sh_bwd_active(const void* params, const void* positions, const int64_t* indexes,
                     const void* camera_pos, int64_t v, int f, int degree, int active_degree, const void* out,
                     const void* grad_out, void* grad_params, void* grad_positions,
                     void* grad_camera_pos, int unique_indexes, int dtype, void* stream);

/* ---- tile mapper -----------------------------------------------------------------------------
 * ms_tile_count replaces tile_overlaps_kernel (mapper/tile_mapper.py:76-86): counts[j] = number
 * of tiles (for gaussian order[j], or j when order is NULL) of the (image_w x image_h, already padded to the tile size) grid that pass the
 * OBB-vs-tile test, restricted to tile rows [tile_row_begin, tile_row_end) (multi-GPU strips;
 * pass 0 and a huge value for the whole image).  points7 is float. */
int ms_tile_count(const float* points7, const int32_t* order, int64_t v, int image_w, int image_h,
                  int tile_size, float alpha_threshold, int tile_row_begin, int tile_row_end,
                  int32_t* out_counts, float* out_ordered_points7 /* (v,7) copy in visiting order, or NULL */,
                  void* stream);

/* Depth pre-sort keys (new design, replaces 2/3 of the reference's 48-bit key sort,
 * tile_mapper.py:156): out_keys[i] = float_bits(depth[i]) (or the 16 bit quantisation of
 * make_sort_key, tile_mapper.py:55-61, when depth16 != 0), out_values[i] = i.  Stable-sorting these
 * pairs yields `order`, the depth order with ties by point index; ms_tile_count / ms_tile_emit then
 * visit the gaussians in that order (counts[j] / keys of gaussian order[j]) so that a stable sort on
 * the TILE ID alone (key_mode 2) reproduces the reference's (tile, depth, point) order.
 * ndc_near > 0 applies ndc_depth (torch_lib/projection.py:120-123) to the camera depth first (in
 * double, from the depth's own dtype), fusing renderer.py:67 into the key generation. */
int ms_depth_sort_keys(const void* depth, int64_t v, int depth16, double ndc_near, double ndc_far,
                       uint32_t* out_keys, int32_t* out_values, int dtype, void* stream);

/* ms_depth_sort_keys + ms_radix_sort_pairs (32 bit keys, all 32 or 16 bits) in one call: the first radix pass makes
 * its keys from `depth` on the fly and takes the item index as value, so no key / value arrays exist before the
 * first scatter.  out_order[j] = index of the j-th gaussian in (depth, index) order, out_sorted_keys its key.
 * (tmp, tmp_bytes): see Conventions; the size ms_radix_sort_pairs reports for v 4-byte keys. */
int ms_depth_argsort(const void* depth, int64_t v, int depth16, double ndc_near, double ndc_far, int dtype,
                     uint32_t* out_sorted_keys, int32_t* out_order, void* tmp, size_t* tmp_bytes, void* stream);

/* cuda_lib.full_cumsum (cuda_lib/full_cumsum.cu:17-67): exclusive scan of n int32 into out[0..n],
 * out[n] = total.  If total_host is not NULL it must be pinned, device-visible host memory and
 * receives the total as well (valid after the stream is synchronised).  (tmp, tmp_bytes): see Conventions. */
int ms_exclusive_scan_i32(const int32_t* in, int64_t n, int32_t* out, int32_t* total_host,
                          void* tmp, size_t* tmp_bytes, void* stream);

/* generate_sort_keys_kernel + make_sort_key (tile_mapper.py:36-66,115-146): for every passing
 * tile of gaussian p = order[j] (or j) writes key and value = p at cum[j]++.
 * key_mode 0: u64 (tile_id << 32) | float_bits(depth[p]);  key_mode 1 (use_depth16): u32
 * (tile_id << 16) | u16(clamp(depth[p],0,1)*65535);  key_mode 2: u32 tile_id only (depth may be
 * NULL; requires `order` = depth order for a depth-sorted result).
 * tile_id = tx + ty * (image_w / tile_size) — NOT limited to 16 bits for modes 0 and 2. */
int ms_tile_emit(const float* points7, const float* depth, const int32_t* order, const int32_t* cum,
                 int64_t v, int image_w, int image_h, int tile_size, float alpha_threshold,
                 int tile_row_begin, int tile_row_end, int key_mode,
                 int points_are_ordered /* points7 is ms_tile_count's ordered copy */,
                 void* out_keys, int32_t* out_values, void* stream);

/* cuda_lib.radix_sort_pairs (cuda_lib/radix_sort_pairs.cu:8-70 = cub::DeviceRadixSort::SortPairs):
 * stable LSD radix sort of n (key, int32 value) pairs on key bits [begin_bit, end_bit),
 * out-of-place, inputs preserved.  key_bytes is 4 or 8 (unsigned order).  (tmp, tmp_bytes): see Conventions. */
int ms_radix_sort_pairs(const void* keys_in, const int32_t* values_in, void* keys_out,
                        int32_t* values_out, int64_t n, int key_bytes, int begin_bit, int end_bit,
                        void* tmp, size_t* tmp_bytes, void* stream);

/* cuda_lib.segmented_sort_pairs (cuda_lib/segmented_sort_pairs.cu:9-73): stable sort of each
 * segment [start_offsets[s], end_offsets[s]) by int32 key, values int32.  Segments are disjoint and may be listed
 * in any order; elements outside every segment (all of them when num_segments == 0) are copied through unchanged. */
int ms_segmented_sort_pairs(const int32_t* keys_in, const int32_t* values_in, int32_t* keys_out,
                            int32_t* values_out, int64_t n, const int64_t* start_offsets,
                            const int64_t* end_offsets, int64_t num_segments, void* stream);

/* find_ranges_kernel (tile_mapper.py:93-112): out_ranges (num_tiles, 2) int32 = [first, last+1)
 * of each tile id (= key >> tile_shift) in the sorted key list; empty tiles get [0, 0).  The
 * function zero-fills out_ranges itself.  0 <= tile_shift <= 8 key_bytes (the whole width: every key is tile 0); ids
 * >= num_tiles are ignored. */
int ms_find_ranges(const void* sorted_keys, int64_t k, int key_bytes, int tile_shift,
                   int64_t num_tiles, int32_t* out_ranges, void* stream);

/* Per-tile depth sort behind a tile-only sort (the last stage of the direct-order mapper, csrc/tile_sort.hip;
 * together with a stable sort of the overlaps on their tile id alone it replaces the reference's 6-pass sort of the
 * whole 64 bit key, tile_mapper.py:148-170, and gives the same order).  payload (K) u64 words
 * key32(depth) << 32 | point index, grouped by tile; tile_ranges (num_tiles, 2): the [first, last + 1) run of each
 * tile.  On return every run of out_overlap_to_point (K) holds the run's point indices in (depth key, point index)
 * order, the order of the payload words themselves.  out_overlap_to_point is output only and every entry inside a
 * range is written: a run of one entry, or of one depth key, has no order to find but is still copied out.  `payload`
 * is scratch afterwards (long runs are sorted through it); `scratch`: K more u64 words. */
int ms_tile_payload_sort(const int32_t* tile_ranges, int64_t num_tiles, uint64_t* payload,
                         int32_t* out_overlap_to_point, uint64_t* scratch, void* stream);

/* The direct-order mapper, from the scanned overlap counts to the lists, with no host read in it: the launch sequence
 * ms_frame_map_raster runs when ms_frame_desc.mapper is MS_MAPPER_DIRECT and map_to_tiles(method='direct') runs on its
 * own.  The overlaps are emitted in storage order as two streams — tile ids of 2 bytes (4 when the image has more than
 * 65 536 tiles) and payload words key32(depth) << 32 | point index — sorted by tile id with the stable radix passes of
 * ms_radix_sort_pairs, ranged, and every tile's run of payload words is sorted as it is (ms_tile_payload_sort).
 * key32 is the sort key of ms_depth_sort_keys: float bits of the depth, of its ndc value when ndc_near > 0
 * (torch_lib/projection.py:120-123), or the 16 bit quantisation when depth16 != 0; depth is float or double
 * (depth_dtype).  The lists are in (tile, key32, point index) order: those of the reference's sort of the whole key
 * (tile_mapper.py:148-170) with ties in point order.
 * points7 (v, 7) float; cum (v + 1) from ms_exclusive_scan_i32 over the counts of ms_tile_count (a gaussian whose
 * count is zero emits nothing); image_w / image_h padded to the tile size.  k_capacity: entries of
 * out_overlap_to_point.  out_tile_ranges (tiles, 2), written whole.  out_counters: 8 int32 on the device —
 * [0] = K = cum[v], [1] = K when K <= k_capacity, else 0, [2] = 1 on that overflow (nothing is emitted, every range is
 * [0, 0)), the rest internal.  (scratch, scratch_bytes): the (tmp, tmp_bytes) of Conventions; 16-byte aligned. */
int ms_map_tiles_direct(const float* points7, const void* depth, int depth_dtype, const int32_t* cum, int64_t v,
                        int image_w, int image_h, int tile_size, float alpha_threshold, int tile_row_begin,
                        int tile_row_end, int depth16, double ndc_near, double ndc_far, int64_t k_capacity,
                        int32_t* out_overlap_to_point, int32_t* out_tile_ranges, int32_t* out_counters,
                        void* scratch, size_t* scratch_bytes, void* stream);

/* ---- rasterizer ------------------------------------------------------------------------------
 * _forward_kernel (rasterizer/forward.py:23-135).  points7 (V,7), features (V,F), tile_ranges
 * (T,2) int32 indexed by tile id = tx + ty * ceil(W/tile), overlap_to_point (K) int32.
 * out_image (H,W,F), out_alpha (H,W), out_visibility (V) (pre-zeroed, used when
 * cfg->compute_visibility) or NULL.  Only tile rows [tile_row_begin, tile_row_end) are rendered. */
int ms_raster_fwd(const void* points7, const void* features, const int32_t* tile_ranges,
                  const int32_t* overlap_to_point, int image_w, int image_h, int f,
                  const ms_raster_config* cfg, void* out_image, void* out_alpha,
                  void* out_visibility, int tile_row_begin, int tile_row_end,
                  int dtype, void* stream);

/* _backward_kernel (rasterizer/backward.py:51-224).  image = forward output, grad_image =
 * dL/dimage.  grad_points7 (V,7), grad_features (V,F) and point_heuristic (V,2) are ACCUMULATED
 * atomically (pre-zero them); each may be NULL to skip that output. */
int ms_raster_bwd(const void* points7, const void* features, const int32_t* tile_ranges,
                  const int32_t* overlap_to_point, const void* image, const void* grad_image,
                  int image_w, int image_h, int f, const ms_raster_config* cfg,
                  void* grad_points7, void* grad_features, void* point_heuristic,
                  int tile_row_begin, int tile_row_end, int dtype, void* stream);

/* Product-path backward (float32, F = 3, plain pdf, alpha blending) in two steps — same semantics as
 * ms_raster_bwd / rasterizer/backward.py:97-224, different organisation (csrc/raster_bwd_scan.hip):
 *
 * ms_raster_bwd_moments ACCUMULATES, per point, one 64-byte row of MS_MOMENT_ROW floats into `moments`
 * (V, MS_MOMENT_ROW), pre-zeroed by the caller, 64-byte aligned:
 *   [0..5]  sum over contributing pixels of q * (1, X', Y', X'^2, X'Y', Y'^2),  q = alpha_pt g dL/dalpha
 *           (backward.py:171-188), (X', Y') = sqrt(log2(e)/2) * the pixel in the splat's normalised frame
 *           (generic.py:311-317)
 *   [6..8]  dL/dfeature = sum w G_c (backward.py:197)
 *   [9..10] with cfg->compute_point_heuristic: sum (dL/dalpha)^2 and sqrt-scaled sum |dL/dmean|_1
 *           (backward.py:190-194)
 *   [11]    with cfg->compute_point_heuristic: sum of the blend weights w = alpha T of the pairs visited (not the ones
 *           backward.py:154 drops behind a pixel's saturation point)
 * Every geometric gradient of gaussian_pdf_with_grad (generic.py:321-336) is a per-splat linear map of these
 * sums; ms_raster_moments_finalize applies it once per point and STORES grad_points7 (V,7), grad_features
 * (V,3) and point_heuristic (V,2) (each may be NULL).
 *
 * deterministic != 0: `moments` is (V, MS_MOMENT_ROW) INT64 (128 bytes per point, pre-zeroed) and the per-patch
 * sums are committed in fixed point with integer atomics, which makes the gradients bitwise reproducible from run
 * to run (float atomics add in arrival order).  The fixed-point unit is chosen per launch from the size of
 * dL/dimage: ms_fixed_point_exponents turns max |grad_image| (one float in device memory, e.g. torch's amax) into
 * the two binary exponents `fixed_exp` (device, int32[2]: sums linear in dL/dimage; the squared prune-cost sum)
 * that both functions then read — no host round trip.  Pass the same flag and exponents to both functions.
 * ms_raster_moments_finalize writes exact zeros for splats that can never blend (alpha or a sigma of 0).
 *
 * Headroom.  ms_fixed_point_exponents looks at max |grad_image| alone: e_main = 36 - e, e_h0 = 36 - 2 e with
 * amax = f 2^e, both clamped to [-100, 100].  A row then holds 2^63 units = amax 2^27 for the linear columns 0..8 and
 * 10 and amax^2 2^29 for column 9, whatever the colours and the number of pixels a splat covers; beyond that it WRAPS,
 * silently (a splat over a 256 x 256 image with colours of ~4000, or over 4096 x 4096 with colours of ~16).  It is kept
 * for existing callers.  ms_fixed_point_exponents_ranged also takes max |feature|, the smallest positive sigma of
 * points7 (stats3_dev: {max |grad_image|, max |feature|, min sigma}, three floats in device memory), the pixel count of
 * the launch window and alpha_threshold, bounds every column from them and coarsens a unit by exactly the bits by which
 * a row could otherwise pass 2^61 units — by none where the units above already fit ("Range of the
 * fixed-point rows"; it assumes alpha <= 1).  Scaling grad_image by 2^k moves both forms' exponents by exactly -k / -2k.
 * A max |feature| that is NaN or infinite is taken as the largest float, a sigma that is not positive and finite as 1. */
#define MS_MOMENT_ROW 16
int ms_fixed_point_exponents(const float* amax_dev, int32_t* out_exp2, void* stream);
int ms_fixed_point_exponents_ranged(const float* stats3_dev, int64_t pixels, float alpha_threshold,
                                    int32_t* out_exp2, void* stream);
int ms_raster_bwd_moments(const void* points7, const void* features, const int32_t* tile_ranges,
                          const int32_t* overlap_to_point, const void* image, const void* grad_image,
                          int image_w, int image_h, const ms_raster_config* cfg, float* moments,
                          int deterministic, const int32_t* fixed_exp, int tile_row_begin, int tile_row_end,
                          void* stream);
int ms_raster_moments_finalize(const void* points7, const float* moments, int deterministic,
                               const int32_t* fixed_exp, int64_t n,
                               float* grad_points7, float* grad_features, float* point_heuristic,
                               void* stream);

/* Splat rows (round 5; no counterpart in the reference, whose kernels index Gaussian2D.vec and the feature array
 * separately — rasterizer/forward.py:85-90, backward.py:118-126).  The product raster kernels (float32, F = 3, plain
 * pdf) can gather each splat from ONE table of MS_SPLAT_ROW floats per point, 64-byte aligned:
 *   [0..6] the points7 row, [7] free (the frame executor stores the depth), [8..10] the colour, [11..15] unused
 * — one 128-byte line per gathered splat instead of two or three (config D: backward -6 %, forward -5 %).  A caller
 * packs the table with ms_splat_rows_pack (depth may be NULL; 0.1 ms for 6 M points) and rasterizes it any number of
 * times: it pays from the second pass over the same projected gaussians on.  (The frame executor, ms_frame_*, whose
 * gaussians change every frame, keeps to the dense arrays: filling the table costs it more than the kernels gain;
 * MS_SPLAT_ROWS=1 in the environment makes it do so for measurements.)  Results
 * are those of ms_raster_fwd / ms_raster_bwd_moments on the same values: the forward bit for bit, the moments up to
 * the order of their float atomics (bit for bit with `deterministic`).  ms_raster_moments_finalize is unchanged (it
 * reads points7).  MS_ERR_UNSUPPORTED for configurations the product kernels do not serve (antialias, no alpha
 * blending for the forward). */
/* Long tile runs (round 5; no counterpart in the reference, whose kernels also walk a tile's list with one thread block,
 * rasterizer/forward.py:77-110).  A tile whose run exceeds 16 384 entries (a zoomed-out view piles the scene onto a few
 * tiles) is cut into segments that separate workgroups blend; one pass per such tile composes the segments front to back
 * (the forward blend is affine in (colour, transmittance)) and leaves, per segment and pixel, the state the backward
 * starts from.  ms_raster_fwd_split = ms_raster_fwd for float32 RGB, plain pdf, alpha blending (else MS_ERR_UNSUPPORTED;
 * with cfg->compute_visibility and out_visibility the segments are walked a second time, from their true start), results equal to it up to the rounding of the re-associated products (1e-7 relative).
 * `split_scratch`: ms_raster_split_scratch_bytes(k_capacity, tile_size) bytes, 256-byte aligned, k_capacity >= the number
 * of overlaps; it carries the plan and the start states to ms_raster_bwd_moments_split (= ms_raster_bwd_moments), which
 * must follow the forward on the same lists.  Scenes without long runs pay three near-empty launches (~10 us). */
/* split_min_run / split_seg_len (round 6): a run is cut when it has MORE than split_min_run entries, into segments of at
 * least split_seg_len entries (rounded up to a multiple of 256, at most 256 segments per tile).  0 = the defaults (16 384;
 * 1024 entries, 4096 at tile 32); values below 256 are raised to 256.  The three calls of a (scratch, forward, backward)
 * group must be given the same pair.  If k_capacity is below the real overlap count the plan may not fit its capacities:
 * it is then dropped as a whole (scratch word [2] = 1) and every tile is rendered by its own workgroup — slower, same
 * results. */
size_t ms_raster_split_scratch_bytes(int64_t k_capacity, int tile_size, int split_min_run, int split_seg_len);
int ms_raster_fwd_split(const float* points7, const float* features, const int32_t* tile_ranges,
                        const int32_t* overlap_to_point, int64_t k_capacity, int image_w, int image_h,
                        const ms_raster_config* cfg, float* out_image, float* out_alpha, float* out_visibility,
                        void* split_scratch, int split_min_run, int split_seg_len, int tile_row_begin, int tile_row_end,
                        void* stream);
int ms_raster_bwd_moments_split(const float* points7, const float* features, const int32_t* tile_ranges,
                                const int32_t* overlap_to_point, int64_t k_capacity, const float* image,
                                const float* grad_image, int image_w, int image_h, const ms_raster_config* cfg,
                                float* moments, int deterministic, const int32_t* fixed_exp, const void* split_scratch,
                                int split_min_run, int split_seg_len, int tile_row_begin, int tile_row_end, void* stream);

/* Measurement hook: the NEXT launch of the product raster backward (ms_raster_bwd_moments*, ms_frame_backward on the
 * moments path) records the two hipEvent_t around its per-tile kernel on the stream it is launched on, then disarms.
 * bench.py times the dominant kernel INSIDE whole frames with it (roofline.kernel_ms); NULL, NULL disarms. */
int ms_probe_raster_bwd(void* start_event, void* stop_event);

#define MS_SPLAT_ROW 16
int ms_splat_rows_pack(const float* points7, const float* depth, const float* colours3, int64_t n, float* rows,
                       void* stream);
int ms_raster_fwd_rows(const float* rows, const int32_t* tile_ranges, const int32_t* overlap_to_point, int image_w,
                       int image_h, const ms_raster_config* cfg, float* out_image, float* out_alpha,
                       float* out_visibility, int tile_row_begin, int tile_row_end, void* stream);
int ms_raster_bwd_moments_rows(const float* rows, const int32_t* tile_ranges, const int32_t* overlap_to_point,
                               const float* image, const float* grad_image, int image_w, int image_h,
                               const ms_raster_config* cfg, float* moments, int deterministic,
                               const int32_t* fixed_exp, int tile_row_begin, int tile_row_end, void* stream);

/* Wide-feature rasteriser (csrc/raster_wide.hip): (V, f) float32 features, 1 <= f <= MS_RASTER_WIDE_MAX_F, blended in
 * ONE pass over the tile lists with the contractions on the f32-input MFMA.  Semantics of ms_raster_fwd / ms_raster_bwd
 * with use_alpha_blending = 1, antialias = 0 on float32 at tile size 16: out_image (H, W, f), out_alpha (H, W), both
 * written whole; the forward has no atomics (two runs are bitwise equal).  The backward ACCUMULATES into grad_points7
 * (V, 7) and grad_features (V, f) (pre-zero them; float atomics); either may be NULL and is then not computed (without
 * grad_points7 the geometry part of the pass is skipped altogether).  cfg->compute_visibility and
 * cfg->compute_point_heuristic are ignored: the wide pass computes neither.  Nothing is read back, allocated or
 * synchronised.  A tile whose range is empty renders zeros.
 * MS_ERR_BAD_ARG: null pointer, a size <= 0, f outside 1..MS_RASTER_WIDE_MAX_F, both gradients NULL;
 * MS_ERR_UNSUPPORTED (after every MS_ERR_BAD_ARG condition): tile size other than 16, antialias, no alpha blending. */
#define MS_RASTER_WIDE_MAX_F 128
int ms_raster_wide_fwd(const float* points7, const float* features, const int32_t* tile_ranges,
                       const int32_t* overlap_to_point, int image_w, int image_h, int f, const ms_raster_config* cfg,
                       float* out_image, float* out_alpha, void* stream);
int ms_raster_wide_bwd(const float* points7, const float* features, const int32_t* tile_ranges,
                       const int32_t* overlap_to_point, const float* image, const float* grad_image, int image_w,
                       int image_h, int f, const ms_raster_config* cfg, float* grad_points7, float* grad_features,
                       void* stream);

/* ---- frame executor --------------------------------------------------------------------------------------------
 * One frame of render_gaussians (renderer.py:23-108) or rasterize (rasterizer/function.py:133-165) as a FIXED launch
 * sequence without host round trips, so that a frame can be enqueued ahead of the GPU and captured in a hipGraph:
 *
 *   - no compaction: the reference compacts the visible gaussians (torch.nonzero + gathers and a host read of V,
 *     perspective/projection.py:147-150).  Here all n gaussians stay in place; a culled one has depth 0, sorts last
 *     in the depth pre-sort, overlaps no tile and gets zero gradient rows.  The tile order (tile, depth bits, point
 *     index) is unchanged because compaction preserves the index order; overlap_to_point holds indexes into the n
 *     input rows.
 *   - the overlap total K stays on the device (the reference reads it back, cuda_lib/full_cumsum.cu:45-46): the
 *     overlap list has a caller-chosen CAPACITY, the sort / range kernels read the live count from `counters`, and
 *     when K exceeds the capacity nothing is emitted (every tile range empty, image = background) and
 *     counters[2] = 1, so a caller that checks can re-run ms_frame_map_raster with larger buffers.
 *
 * ms_frame_layout reports the sizes of the four caller-owned blocks and the offsets of the arrays inside them:
 *   keep_n / keep_k   per-gaussian / per-overlap arrays that the backward pass (and the caller) read
 *   scratch_n / scratch_k   dead once the forward calls returned (stream order)
 * counters (int32[8] at lay.counters in keep_n): [0] K, [1] live K (0 on overflow), [2] overflow flag.
 *
 * ms_frame_project:        the per-gaussian stage alone (camera position, projection, SH colours) into keep_n — what a
 *     rank of the gaussian-sharded multi-GPU step runs on its shard before the exchange.
 * ms_frame_project_count:  camera position, projection, depth pre-sort, overlap count, scan, K (the SH colours are
 *     evaluated by ms_frame_map_raster: nothing before the raster forward needs them, and a host that looks at K
 *     then finds the long SH pass queued behind the K kernel, not in front of it).
 *     projected_input != 0 (2-D path, splats received for a multi-GPU strip): in->points7 / depth / colours are
 *     used as they are and nothing is culled by depth.  k_host (pinned host int32, may be NULL) receives K;
 *     k_event (hipEvent_t, may be NULL) is recorded right after the kernel that writes it.
 * ms_frame_map_raster:     SH colours, emission, stable sort on the tile id, tile ranges, raster forward.
 * ms_frame_backward:       raster backward + ONE pass over the gaussians (moment rows -> 2D gradients -> projection
 *     backward -> SH backward; csrc/gaussian_bwd.hip).  ms_frame_uses_moments(desc) != 0: the product raster
 *     backward runs and g->moments (n, MS_MOMENT_ROW) must be zero on entry and is zero again on return;
 *     otherwise g->grad_points7 / grad_colours are zero-initialised accumulators of ms_raster_bwd. */
/* Two launch sequences build the same overlap_to_point / tile_ranges (same order, ties included):
 *   MS_MAPPER_DIRECT   overlaps emitted in storage order as a 2-byte tile id (4 beyond 65 536 tiles) and an 8-byte
 *                      payload depth key << 32 | point, stable sort on the tile bits, per-tile depth sort of the
 *                      payload runs (ms_map_tiles_direct).  68 bytes moved per overlap, nothing per gaussian
 *                      beyond the count / emit passes: the faster one up to about 3.5 overlaps per gaussian.
 *   MS_MAPPER_PRESORT  gaussians sorted by depth first (4 passes over n pairs), overlaps counted and emitted in that
 *                      order, stable sort of (tile id, point) on the tile bits: 52 bytes per overlap.
 * The environment variable MS_MAPPER=direct|presort overrides the field for a whole process (A/B runs). */
#define MS_MAPPER_DIRECT 0
#define MS_MAPPER_PRESORT 1

typedef struct ms_frame_desc {
  uint32_t struct_size;            /* sizeof(ms_frame_desc) of the header the caller was compiled against ... */
  uint32_t abi_version;            /* ... and its MS_VERSION: another size or ABI generation is refused (MS_ERR_ABI) */
  int64_t n;                       /* gaussians = rows of every per-gaussian array */
  int64_t k_capacity;              /* rows of the overlap list */
  int32_t image_w, image_h;
  int32_t dtype;                   /* MS_F32 / MS_F64 */
  int32_t f;                       /* colour channels of the rasterizer (1..4) */
  int32_t sh_degree;               /* -1: `feature` / `colours` are (n, f) colours; 0..3: `feature` is (n, f, (deg+1)^2) */
  int32_t depth16;                 /* use_depth16 sort keys */
  int32_t tile_row_begin, tile_row_end;   /* multi-GPU strip (0, INT32_MAX: whole image) */
  int32_t projected_input;
  int32_t mapper;                  /* MS_MAPPER_DIRECT / MS_MAPPER_PRESORT: the same in every call of a frame */
  int32_t split_long_runs;         /* != 0: long tile runs are cut into segments blended by separate workgroups
                                      (ms_raster_fwd_split; float32 RGB product kernels, ignored otherwise); the same
                                      in every call of a frame.  1: runs above 16 384 entries; > 1: runs above that
                                      many entries (ms_raster_fwd_split's split_min_run).  Costs three near-empty
                                      launches when there is no such run: set it for scene shapes that showed one
                                      (ms_frame_inputs.longest_run_host) */
  int32_t split_seg_len;           /* 0: the default segment length; else ms_raster_fwd_split's split_seg_len */
  int32_t sh_active_bands;         /* 0: every stored SH band; 1 .. sh_degree + 1: only that many bands (active degree + 1)
                                      are evaluated and differentiated — colours of `feature` sliced to them, the
                                      gradient of the other coefficients written as zeros (ms_sh_fwd_active); the same
                                      in every call of a frame.  Refused above sh_degree + 1 and without SH */
  double near_plane, far_plane, blur_cov, clamp_margin;
  ms_raster_config raster;
} ms_frame_desc;

typedef struct ms_frame_layout {
  size_t keep_n_bytes, scratch_n_bytes, keep_k_bytes, scratch_k_bytes;
  /* keep_n */
  size_t points7, depth, colours, points7_f32, camera_position, counters, tile_ranges;
  /* scratch_n */
  size_t sorted_keys, order, counts, cum, ordered_points, tmp_n;
  /* keep_k */
  size_t overlap_to_point;
  /* scratch_k */
  size_t keys, values, keys_sorted, tmp_k;
  /* keep_n, behind tile_ranges: the splat-row table (64 bytes per gaussian) of a process started with MS_SPLAT_ROWS=1;
   * 256 unused bytes otherwise */
  size_t splat_rows;
  /* keep_k, behind overlap_to_point: plan and start states of the long-run segments (ms_frame_desc.split_long_runs);
   * 256 unused bytes otherwise */
  size_t split_scratch;
} ms_frame_layout;

typedef struct ms_frame_inputs {
  uint32_t struct_size;            /* sizeof(ms_frame_inputs) */
  uint32_t reserved;
  const void *position, *log_scaling, *rotation, *alpha_logit, *feature, *T_camera_world, *projection;
  const void *points7, *depth, *colours;       /* projected_input */
  /* optional (pinned host int32, device-visible): when a tile's run exceeds 16384 entries, ms_frame_map_raster writes
   * its length there (one of them if there are several; never written otherwise) — the per-tile sort of
   * MS_MAPPER_DIRECT and the product raster forward do.  Such a run is sorted by ONE workgroup at ~12 ns per entry and
   * rasterized by one workgroup: a caller that finds the word set switches the scene shape to MS_MAPPER_PRESORT, whose
   * cost does not depend on how the overlaps are spread over the tiles, and sets split_long_runs
   * (taichi_splatting_amd/frame.py does). */
  int32_t* longest_run_host;
  /* optional hipEvent_t: ms_frame_map_raster makes `stream` wait for it right before the raster forward — the first kernel
   * of the frame that reads `colours` (projected_input frames).  A multi-GPU rank step records it behind the collective
   * that delivers the colours, so the mapper overlaps that transfer.  NULL: no wait. */
  void* colours_ready_event;
} ms_frame_inputs;

enum { MS_BACKWARD_ALL = 0, MS_BACKWARD_GAUSSIANS = 1, MS_BACKWARD_RASTER = 2 };

typedef struct ms_frame_grads {
  uint32_t struct_size;            /* sizeof(ms_frame_grads) */
  uint32_t reserved;
  const void* image;               /* forward image (H, W, f) */
  const void* grad_image;
  const void *extra_points7, *extra_depth, *extra_colours;   /* dL/d(frame's own per-gaussian outputs), may be NULL */
  void* moments;
  int32_t deterministic;
  int32_t stage;                   /* MS_BACKWARD_ALL, or one half of it around a multi-GPU gradient collective:
                                      MS_BACKWARD_RASTER stops after the raster backward and STORES the 2D-boundary
                                      gradients in grad_points7 / grad_colours; MS_BACKWARD_GAUSSIANS runs only the
                                      per-gaussian pass on the gradients GIVEN in those two arrays */
  const int32_t* fixed_exp;
  void *grad_points7, *grad_colours;   /* moments path: optional stores of the summed 2D-boundary gradients */
  void *grad_position, *grad_log_scaling, *grad_rotation, *grad_alpha_logit, *grad_feature, *grad_camera;
  void* point_heuristic;           /* (n, 2), written (moments path) or accumulated (zero-initialised) */
  void* point_visibility;          /* (n,) or NULL.  Moments path with raster.compute_point_heuristic, MS_BACKWARD_ALL: for
                                      every gaussian that passed the projection's culling, WRITES the sum of the blend weights
                                      of the (pixel, splat) pairs the raster backward visited: the visibility of
                                      forward.py:127-128 WITHOUT the pairs behind a pixel's saturation point (backward.py:154
                                      drops them, the forward keeps adding them: at most 1 - saturate_threshold per pixel).
                                      A training loop that accepts that difference can run its forward without
                                      out_visibility.  Ignored on the other paths (ms_frame_uses_moments() tells which runs) */
  int32_t boundary_stride;         /* 0: grad_points7 (n, 7) and grad_colours (n, f) are two dense arrays.  > 0: both are
                                      columns of ONE row-major array with this many floats per row (the return buffer of a
                                      multi-GPU rank step: grad_colours = grad_points7 + 7, stride 7 + f) — float32 frames,
                                      MS_BACKWARD_RASTER on the moments path (stores) and MS_BACKWARD_GAUSSIANS (reads) only */
  int32_t gather_world;            /* MS_BACKWARD_GAUSSIANS, > 0: the 2D-boundary gradient of gaussian i is the SUM of the rows
                                      gather_slots[i * gather_world + c], c < (gather_route[i] >> 16), of gather_rows
                                      (rows of boundary_stride floats: [d packed 2D | d colour]; slot < 0: no row) — the
                                      receive buffer of a rank step's reverse exchange read in place: no return pass, no
                                      home array.  grad_points7 / grad_colours are then unused */
  const void* gather_rows;
  const int32_t* gather_slots;     /* out_slots of ms_strip_route_pack_slots */
  const int32_t* gather_route;     /* out_route of ms_strip_route_count */
  int32_t boundary_form;           /* form of the 2D-boundary gradient rows that MS_BACKWARD_RASTER stores (moments path) and
                                      MS_BACKWARD_GAUSSIANS reads.  0 = MS_BOUNDARY_AXIS_SIGMA: d(packed 2D gaussian) as the
                                      reference's rasterizer returns it, [d mean (2) | d axis (2) | d sigma (2) | d alpha].
                                      1 = MS_BOUNDARY_COVARIANCE: [d mean (2) | dL/d(a, b, c) of the 2D covariance
                                      [[a, b], [b, c]] (3) | 0 | d alpha] — the same 7 columns.  The plain gaussian pdf depends
                                      on (axis, sigma) only through the covariance; handed over in this form the gradient
                                      never passes through the derivative of the eigen-decomposition (no division by
                                      l1 - l2: float32 rows of nearly isotropic splats keep their digits), and rows of
                                      one gaussian from several strips / ranks simply add.  Multi-GPU rank steps use 1. */
  int32_t grad_image_broadcast;    /* != 0 (moments path only): grad_image points to ONE pixel's f values, used for every pixel —
                                      dL/dimage of a sum / mean loss is an expanded scalar, which the caller need not
                                      materialise as an (H, W, f) array (50 MB at 2048^2 written and read back otherwise) */
} ms_frame_grads;

enum { MS_BOUNDARY_AXIS_SIGMA = 0, MS_BOUNDARY_COVARIANCE = 1 };

int ms_frame_layout_query(const ms_frame_desc* desc, ms_frame_layout* out);
int ms_frame_uses_moments(const ms_frame_desc* desc, int deterministic);
int ms_frame_project(const ms_frame_desc* desc, const ms_frame_inputs* in, void* keep_n, void* stream);
int ms_frame_project_count(const ms_frame_desc* desc, const ms_frame_inputs* in, void* keep_n, void* scratch_n,
                           int32_t* k_host, void* k_event, void* stream);
/* The SH colours of a frame (the second half of ms_frame_project: camera position = inverse(T_camera_world)[:3, 3],
 * perspective/params.py:78-80, then evaluate_sh_at, indexed_spherical_harmonics.py:119-134, into keep_n) as a call of its
 * own, so that a caller can enqueue it on ANOTHER stream behind ms_frame_project_count (it reads the depths the projection
 * wrote) and beside the mapper's launches of ms_frame_map_raster: that call, given ms_frame_inputs.colours_ready_event
 * (an event recorded behind this one), skips the colours and waits for the event in front of the raster forward.  Frames
 * with sh_degree >= 0 and their own projection only; not with the splat-row table. */
int ms_frame_sh_colours(const ms_frame_desc* desc, const ms_frame_inputs* in, void* keep_n, void* stream);
int ms_frame_map_raster(const ms_frame_desc* desc, const ms_frame_inputs* in, void* keep_n, void* scratch_n,
                        void* keep_k, void* scratch_k, void* out_image, void* out_alpha, void* out_visibility,
                        void* stream);
int ms_frame_backward(const ms_frame_desc* desc, const ms_frame_inputs* in, void* keep_n, void* keep_k,
                      const ms_frame_grads* g, void* stream);

/* ---- optimiser step ------------------------------------------------------------
 * Moment update of the fractional (visibility-weighted) Adam (kind 0, optim/fractional_adam.py:8-86)
 * and LaProp (kind 1, optim/fractional_laprop.py:8-86) for the m_count visible points listed in
 * indexes: reads grad[idx] (N,D), the per-point step weight (m_count) and total_weight[idx] (N),
 * updates m (N,D) and v ((N,D), or (N,) when vector != 0: one second moment per point from the
 * squared gradient norm) in place and writes lr_step (m_count, D), float32. */
int ms_fractional_step(int kind, int vector, float* lr_step, const int64_t* indexes,
                       const float* weight, float* m, float* v, const float* total_weight,
                       const float* grad, int64_t m_count, int d, float lr, float beta1,
                       float beta2, float eps, int bias_correction, void* stream);

/* Fused per-group update (optim/fractional.py:108-156,176-195 + the gradient pre-scaling of
 * optim/visibility_aware.py:95-104) for the m_count visible rows listed in indexes, in one pass:
 *   g = grad[idx] * grad_scale[i];  local_vector (group_type 2, d = 2 or 3): g = basis[i]^-1 g;
 *   moments m / v updated as in ms_fractional_step (group_type 0: v is (N,D); 1, 2: v is (N,));
 *   step clamped to +-lr*clip (clip < 0: off); local_vector: step = basis[i] step; *= mask_lr[j];
 *   *= point_lr[idx]; non-finite -> 0;  param[idx] -= step * (1 - exp(-2 weight[i])).
 * grad_scale (m_count), basis (m_count, d, d), mask_lr (d), point_lr (N) may be NULL.  float32, d <= 256. */
int ms_fractional_update(int kind, int group_type, float* param, const float* grad, float* m, float* v,
                         const int64_t* indexes, const float* weight, const float* total_weight,
                         const float* grad_scale, const float* basis, const float* mask_lr,
                         const float* point_lr, int64_t m_count, int d, float lr, float beta1,
                         float beta2, float eps, float clip, int bias_correction, void* stream);

/* All parameter groups of one optimiser step in ONE launch (round 6; the reference loops over its groups on the host,
 * optim/fractional.py:176-195, optim/visibility_aware.py:86-104).  Each group is what ms_fractional_update takes;
 * indexes / weight / total_weight / grad_scale are shared by the groups, as they are in the reference's step().
 * Rows whose length is a multiple of 4 floats (16-byte aligned arrays) move as 16-byte pieces.  indexes == NULL
 * means rows 0 .. m_count - 1, and then a row with weight[i] < 0 (or NaN) is skipped: the dense mode of
 * ms_optim_visibility_weights.  With an index list every listed row is updated, a negative weight included
 * (beta^w > 1, as the reference's beta ** w).  Every group is checked before the first launch: an error return
 * leaves every array as it was.  `groups` is a HOST array. */
typedef struct ms_optim_group {
  uint32_t struct_size;            /* sizeof(ms_optim_group) */
  int32_t group_type;              /* 0 scalar, 1 vector, 2 local_vector */
  float* param;                    /* (N, d) */
  const float* grad;               /* (N, d) */
  float* m;                        /* (N, d) first moment */
  float* v;                        /* second moment: (N, d) for scalar groups, (N,) otherwise */
  const float* basis;              /* local_vector: (m_count, d, d), else NULL */
  const float* mask_lr;            /* (d) or NULL */
  const float* point_lr;           /* (N) or NULL */
  int32_t d;
  int32_t bias_correction;
  float lr, beta1, beta2, eps;
  float clip;                      /* < 0: off */
  float reserved;
} ms_optim_group;
int ms_optim_step_groups(int kind, const ms_optim_group* groups, int num_groups, const int64_t* indexes,
                         const float* weight, const float* total_weight, const float* grad_scale, int64_t m_count,
                         void* stream);

/* Step weights of the visibility-aware optimisers in one pass (optim/visibility_aware.py:35-52 update_visibility and
 * :86-104): for the m_count rows listed in indexes, running_vis <- ((1 - beta) v^4 + beta running_vis^4)^(1/4),
 * out_weight = v / max(running_vis, floor_eps), total_weight += out_weight, out_grad_scale = 1 / (v + vis_smooth)
 * (out_grad_scale may be NULL).  indexes == NULL (dense mode): row i is point i, and a point with
 * visibility <= skip_threshold is left untouched and gets out_weight = -1 (which ms_optim_step_groups skips in
 * its dense mode) — the reference's `visible = (visibility > 1e-8).nonzero()` without the host
 * synchronisation (examples/fit_image_gaussians.py:118-119). */
int ms_optim_visibility_weights(const int64_t* indexes, const float* visibility, int64_t m_count, float vis_beta,
                                float vis_smooth, float floor_eps, float skip_threshold, float* running_vis,
                                float* total_weight, float* out_weight, float* out_grad_scale, void* stream);

/* ---- Morton codes --------------------------------------------------------------------
 * out_codes[i] = 63-bit Z-order code of points3[i] (N, 3 float32) on the grid of cell size inc3_host anchored at
 * lower3_host (3 floats each, host memory) with `size` cells per axis (<= 2^21): cell = clamp((p - lower) / inc,
 * 0, size - 1) truncated; x, y, z bits interleaved from bit 0 (misc/morton_sort.py:25-33,56-70,94-99).
 * Sort with ms_radix_sort_pairs (key_bytes 8) for misc/morton_sort.py:113-119 argsort. */
int ms_morton_codes64(const float* points3, int64_t n, const float* lower3_host, const float* inc3_host,
                      uint32_t size, uint64_t* out_codes, void* stream);

/* ---- k nearest neighbours of a 3-D point set (no reference counterpart; upstream trainers use simple_knn) ----
 * Exact: out_dist2 (N, k) float32 = the k smallest squared distances from points3[i] (N, 3 float32) to the OTHER points
 * of the same array, ascending; out_index (N, k) = their indices.  Self is excluded by index, so a duplicate point is a
 * neighbour at distance 0; a missing neighbour (N - 1 < k) is +inf / -1.  1 <= k <= 8, N < 2^31.
 * d2 = (dx dx + dy dy) + dz dz on float32 differences, unfused: out_dist2 is bitwise independent of `order`.
 * order: a permutation of 0..N-1 (device), normally the argsort of ms_morton_codes64 by ms_radix_sort_pairs: consecutive
 * runs of MS_KNN_BLOCK points in that order are the blocks whose boxes prune the search.  The results do not depend on
 * which permutation, only the speed does (an entry outside 0..N-1 is clamped: wrong results, no stray access).
 * out_stats: NULL, or a device int64[2] to which the search ADDS [blocks scanned x queries of the wave, point-query
 * distance evaluations] (the caller zeroes it); brute force would evaluate N (N - 1).
 * (tmp, tmp_bytes): see Conventions.  No host read, allocation or synchronisation: capturable into a graph.
 * MS_ERR_BAD_ARG names the argument: n < 0, n >= 2^31, k, null points3 / order / out_dist2 with n > 0, null tmp_bytes,
 * and — this function only — a *tmp_bytes that is too small.  n == 0 returns 0 without a launch. */
#define MS_KNN_BLOCK 256
int ms_knn_points(const float* points3, const int32_t* order, int64_t n, int k,
                  float* out_dist2, int32_t* out_index /* may be NULL */, int64_t* out_stats /* may be NULL */,
                  void* tmp, size_t* tmp_bytes, void* stream);

/* ---- k nearest points of ANOTHER set (csrc/knn_query.hip; an addition: Chamfer distance and F-score of a mesh against a
 * ground-truth cloud, colour transfer between clouds, "farther than d from the surface") ----
 * Exact: out_dist2 (N, k) float32 = the k smallest squared distances from queries3[i] (N, 3 float32) to the M rows of
 * points3 (M, 3 float32), ascending; out_index (N, k) = the points' original indices; both rows are written at the
 * query's ORIGINAL index.  Nothing is excluded: a query that coincides with a point finds it at distance 0.  With M < k
 * the missing entries are +inf / -1; M == 0 (every entry missing) and N == 0 (no launch) are legal.  1 <= k <= 8,
 * M, N < 2^31.  d2 is the function of ms_knn_points, (dx dx + dy dy) + dz dz on float32 differences, unfused: a distance
 * is a pure function of its pair, so out_dist2 is bitwise independent of point_order, query_order and query_hint; under
 * ties any valid index may be returned.
 * point_order (M) and query_order (N): permutations (device), normally the Morton argsorts of the two sets on ONE grid
 * (ms_morton_codes64 with the common bounding box + ms_radix_sort_pairs).  Runs of MS_KNN_BLOCK points in point_order are
 * the blocks whose boxes prune the search; the 64 queries of a wave are consecutive in query_order.  query_hint: NULL,
 * or (N) int32 where query_hint[i] is the position in point_order near which the query at position i of query_order
 * should start (normally searchsorted(sorted point codes, sorted query codes)); it is clamped to 0 .. M - 1, and a wave
 * seeds from the block of its middle active lane's hint.  NULL stands for i M / N.  Every block is still considered and
 * every pruning test is <=: orders and hint decide the speed only (an order entry outside its range is clamped: wrong
 * results, no stray access).
 * out_stats: NULL, or a device int64[2] to which the search ADDS [blocks scanned x queries of the wave, point-query
 * distance evaluations] (the caller zeroes it); brute force would evaluate M N.
 * (tmp, tmp_bytes): see Conventions (sized by M; aligned to 16 bytes).  No host read, allocation or synchronisation:
 * capturable into a graph.  MS_ERR_BAD_ARG names the argument: m or n < 0 or >= 2^31, k, a null points3 / point_order
 * with m > 0, a null queries3 / query_order / out_dist2 with n > 0, null tmp_bytes. */
int ms_knn_query(const float* points3, const int32_t* point_order, int64_t m,
                 const float* queries3, const int32_t* query_order, const int32_t* query_hint /* may be NULL */, int64_t n,
                 int k, float* out_dist2, int32_t* out_index /* may be NULL */, int64_t* out_stats /* may be NULL */,
                 void* tmp, size_t* tmp_bytes, void* stream);

/* ---- camera position ----------------------------------------------------------------------------------
 * out_position3 = inverse(T_camera_world)[0:3, 3] for a row-major 4x4 (perspective/params.py:62-65), one
 * launch instead of a device-side LU. */
int ms_camera_position(const void* t_camera_world, void* out_position3, int dtype, void* stream);

/* ---- multi-GPU: routing projected splats to tile-row strips -----------------------------
 * New design, no reference counterpart (the reference renders on one GPU).  Rank r renders the tile rows
 * [bounds[r], bounds[r+1]); a projected splat goes to every rank whose strip meets the tile-row span of
 * the mapper's grid query (taichi_lib/grid_query.py:10-40), i.e. a stable multi-way split by destination.
 * float32 only.
 *
 * ms_strip_route_blocks: number of 256-splat blocks B of the split (scratch: out_block_counts is
 *   world x B int32).
 * ms_strip_route_count: out_route[i] = first_rank | copies << 16; out_block_counts = per-(rank, block)
 *   exclusive slot offsets inside the rank's bucket; out_send_counts[r] (int64, device) = splats routed
 *   to rank r = the all-to-all split sizes.  bounds_host: world + 1 ints in host memory.
 * ms_strip_route_pack: writes the send buffer, buckets in rank order and local index order inside a
 *   bucket: out_rows (S, 9 + f) = [packed 2D (7) | colour (f) | depth | global id as int32 bits], global
 *   id = (ids ? ids[i] : i) + index_offset; out_send_index[slot] = i (to sum the returned gradients).
 * ms_strip_unpack: splits received rows into the arrays the mapper / rasterizer consume.
 * ms_strip_return_grads: backward of the exchange on the sending side: back_rows (S, 7 + f) =
 *   [d packed 2D | d colour] of every slot of the send buffer, summed into the zero-initialised
 *   grad_points7 (V, 7) / grad_features (V, f) of the local splats (grad[send_index[slot]] += row);
 *   route = out_route of ms_strip_route_count (splats with one copy are stored, not accumulated); slots with
 *   send_index < 0 (unused rows of fixed buckets) are skipped. */
int ms_strip_route_blocks(int v);
int ms_strip_route_count(const float* points7, const float* depth /* NULL, or (v): rows with depth <= 0 are culled */,
                         int v, int image_h, int tile_size, float alpha_threshold,
                         const int32_t* bounds_host, int world, int32_t* out_route,
                         int32_t* out_block_counts, int64_t* out_send_counts, void* stream);
/* bucket_capacity > 0: FIXED buckets — destination r owns rows [r * capacity, (r + 1) * capacity) of out_rows, so
 * the all-to-all has equal splits the host knows without reading the counts back (sync-free rank step, HIP-graph
 * capture).  The caller zero-fills out_rows (an all-zero row is a splat with alpha 0: it overlaps no tile and gets
 * no gradient) and fills out_send_index with -1 first; rows beyond a bucket's capacity are dropped and
 * *overflow_flag (device int32, may be NULL) is set.  bucket_capacity == 0: buckets of exactly send_counts[r] rows. */
int ms_strip_route_pack(const float* points7, const float* features, const float* depths,
                        const int64_t* ids, int f, int v, int world, int64_t index_offset,
                        const int32_t* route, const int32_t* block_offsets, const int64_t* send_counts,
                        int64_t bucket_capacity, int32_t* overflow_flag,
                        float* out_rows, int64_t* out_send_index, void* stream);
/* the same, and out_slots[i * world + c] (int32, may be NULL) = row of out_rows that holds copy c of local splat i
 * (c < copies of out_route), -1 for a copy dropped by a full bucket: what ms_frame_grads.gather_slots reads */
int ms_strip_route_pack_slots(const float* points7, const float* features, const float* depths,
                              const int64_t* ids, int f, int v, int world, int64_t index_offset,
                              const int32_t* route, const int32_t* block_offsets, const int64_t* send_counts,
                              int64_t bucket_capacity, int32_t* overflow_flag,
                              float* out_rows, int64_t* out_send_index, int32_t* out_slots, void* stream);
/* the same with the colours in a buffer of their own (round 6: the forward exchange as TWO collectives, so that the
 * receiving strip's mapper — which reads geometry only — runs while the colours are still on the links):
 * out_geometry_rows (S, 9) = [packed 2D (7) | depth | global id bits], out_colour_rows (S, f); both zero-filled by the
 * caller for fixed buckets.  ms_strip_unpack(rows9, m, 0, points7, NULL, depths, ids) splits the geometry rows; the
 * colour rows ARE the (m, f) colour array the rasterizer reads (ms_frame_inputs.colours +
 * ms_frame_inputs.colours_ready_event). */
int ms_strip_route_pack_split(const float* points7, const float* features, const float* depths,
                              const int64_t* ids, int f, int v, int world, int64_t index_offset,
                              const int32_t* route, const int32_t* block_offsets, const int64_t* send_counts,
                              int64_t bucket_capacity, int32_t* overflow_flag, float* out_geometry_rows,
                              float* out_colour_rows, int64_t* out_send_index, int32_t* out_slots, void* stream);
int ms_strip_unpack(const float* rows, int64_t m, int f, float* out_points7, float* out_features,
                    float* out_depths, int64_t* out_ids, void* stream);
int ms_strip_return_grads(const float* back_rows, const int64_t* send_index, const int32_t* route,
                          int f, int64_t s, float* grad_points7, float* grad_features, void* stream);
/* the same into ONE zero-initialised (V, 7 + f) array of rows [d packed 2D | d colour] (one line per splat instead of
 * two; ms_frame_grads.boundary_stride = 7 + f hands it to the per-gaussian pass) */
int ms_strip_return_rows(const float* back_rows, const int64_t* send_index, const int32_t* route,
                         int f, int64_t s, float* grad_rows, void* stream);

/* ---- Densification: prune and split the rows of every per-point array of a training state (csrc/densify.hip) --------
 * Replaces the torch chain of the reference's training loop — params[mask] / torch.cat per tensor and per optimiser
 * state tensor (optim/parameter_class.py:215-248, examples/fit_image_gaussians.py:190-231) and the child geometry of
 * misc/renderer2d.py:60-131 — by a fixed launch sequence with one host read (the new row count).
 *
 * Destination layout: [kept rows in storage order | children grouped by parent in storage order, `children` per
 * parent], i.e. torch.cat([x[~(prune | split)], children]).  A row flagged in both masks is pruned.
 *
 * ms_densify_plan: prune / split are n bytes each (non-zero = set).  scan (2 n + 1 int32) receives the exclusive scan
 * of [keep flags | split flags] (scan[i] = destination of kept row i, scan[n] = n_kept, scan[n + i] - n_kept = rank of
 * split parent i).  counts (device, 4 int32) = (n_kept, n_split_parents, n_out, n); counts_host (pinned, device-visible
 * host memory, may be NULL) receives the same, valid after the stream is synchronised.  (tmp, tmp_bytes): see
 * Conventions.  n * children and 2 n + 1 must fit int32.
 * ms_densify_table: the source table over the n_out destination rows: src_row (source row) and child_slot
 * (0 .. children - 1 for a child, -1 for a kept row). */
int ms_densify_plan(const uint8_t* prune, const uint8_t* split, int64_t n, int children, int32_t* scan,
                    int32_t* counts, int32_t* counts_host, void* tmp, size_t* tmp_bytes, void* stream);
int ms_densify_table(const int32_t* scan, int64_t n, int children, int64_t n_out, int32_t* src_row,
                     int32_t* child_slot, void* stream);

/* ms_densify_move: every array of the step in ONE launch.  Destination row r of each array is source row src_row[r];
 * child rows (child_slot[r] >= 0) are zero with child_fill 0 (what append_tensors gives optimiser state,
 * optim/parameter_class.py:236-248) or copy their parent with child_fill 1.  Rows move as 16-byte pieces when
 * row_bytes % 16 == 0 and both bases are 16-byte aligned, as 4-byte pieces otherwise; row_bytes must be a positive
 * multiple of 4 (at most 1 MiB).  A source row outside [0, n_src) is written as zeros.  Every descriptor is checked
 * before the first launch: an error return leaves every array as it was.  `arrays` is a HOST array; src and dst must
 * not overlap. */
typedef struct ms_densify_array {
  uint32_t struct_size;            /* sizeof(ms_densify_array) */
  int32_t child_fill;              /* 0: child rows are zero, 1: child rows copy the parent */
  const void* src;                 /* (n_src, row_bytes) */
  void* dst;                       /* (n_out, row_bytes) */
  int64_t row_bytes;
} ms_densify_array;
int ms_densify_move(const ms_densify_array* arrays, int num_arrays, const int32_t* src_row, const int32_t* child_slot,
                    int64_t n_src, int64_t n_out, void* stream);

/* Child geometry, in place on rows first .. first + count - 1 of the destination arrays, which hold copies of the
 * parents (ms_densify_move with child_fill 1); row first + c is child c % children of parent c / children.
 * z (count, 2 | 3): unit-space samples; scale (count / children, 2 | 3): per-parent factor of the children's
 * scaling, NULL = 1; depth_offset (count), NULL = 0.  float32.
 * 2-D (misc/renderer2d.py:36-43,56-67,101-103): position += [v1 s1 | v2 s2] z with v1 = rotation / |rotation|,
 * v2 = (-v1.y, v1.x), s = max(exp(log_scaling), 1e-4);  log_scaling += log(scale);
 * depths = max(depths + depth_offset, 1e-6) (depths may be NULL).
 * 3-D: position += R(q / |q|) (exp(log_scaling) * z), xyzw quaternion as in the projection
 * (taichi_lib/generic.py:408-416);  log_scaling += log(scale).
 * A zero offset / a factor of exactly 1 leaves the value as it is, bit for bit. */
int ms_densify_split2d(float* position, float* log_scaling, const float* rotation, float* depths, int64_t first,
                       int64_t count, int children, const float* z, const float* scale, const float* depth_offset,
                       void* stream);
int ms_densify_split3d(float* position, float* log_scaling, const float* rotation, int64_t first, int64_t count,
                       int children, const float* z, const float* scale, void* stream);

/* ---- Photometric loss: (1 - lambda) L1 + lambda (1 - SSIM), forward and backward (csrc/loss.hip) ---------------------
 * An addition, not a replacement: the reference has no loss (its demo calls torch's mse_loss).  image and target are
 * contiguous (H, W, C) arrays of `dtype`, the layout the rasterizer writes and its backward reads; 1 <= C <= 4.
 *
 * Per channel, with G the separable 11-tap window exp(-k^2 / (2 1.5^2)) normalised to sum 1, C1 = 0.01^2, C2 = 0.03^2:
 *   mu1 = G*x   mu2 = G*y   s11 = G*x^2 - mu1^2   s22 = G*y^2 - mu2^2   s12 = G*xy - mu1 mu2
 *   ssim = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s11 + s22 + C2))
 *   loss = (1 - lambda) mean|x - y| + lambda (1 - mean ssim)
 * padding MS_PAD_SAME zero-pads like conv2d(padding = 5): the ssim map is (H, W, C).  MS_PAD_VALID keeps the elements
 * whose window lies inside the image: the map is (H - 10, W - 10, C) and H, W >= 11 is required.  mean|x - y| is over
 * the H W C image elements, mean ssim over the map elements.
 *
 * ms_photometric_fwd: out_loss (device, 3 values of `dtype`) = {loss, mean|x - y|, mean ssim}.  map_a, map_b, map_c:
 * all three NULL, or three arrays of the ssim map's shape that receive, per element, what the backward needs:
 * A = d ssim/d mu1 - 2 mu1 B - mu2 C,  B = d ssim/d s11,  C = d ssim/d s12.  tmp holds one pair of partial sums
 * (double) per workgroup, added in a fixed order by a second kernel: the result is bit-reproducible (no atomics).
 * (tmp, tmp_bytes): see Conventions.
 * ms_photometric_bwd: grad_image (H, W, C) =
 *   grad_out * [ (1 - lambda) / (H W C) sign(x - y) - lambda / (map elements) (G*A + 2 x G*B + y G*C) ],
 * sign(0) = 0; the maps are those of a forward with the same sizes and padding (`valid`: absent map elements count as
 * zero, the full correlation).  grad_out is ONE value of `dtype` in DEVICE memory: neither call reads back to the host.
 * There is no gradient for target.
 * MS_ERR_BAD_ARG: null pointer, H, W <= 0, C outside 1..4, unknown padding, `valid` with a side under 11, lambda
 * outside [0, 1]; MS_ERR_UNSUPPORTED: unknown dtype; MS_ERR_TMP_TOO_SMALL. */
enum { MS_PAD_SAME = 0, MS_PAD_VALID = 1 };
int ms_photometric_fwd(const void* image, const void* target, int H, int W, int C, int dtype, int padding,
                       double lambda, void* map_a, void* map_b, void* map_c, void* tmp, size_t* tmp_bytes,
                       void* out_loss, void* stream);
int ms_photometric_bwd(const void* image, const void* target, const void* map_a, const void* map_b, const void* map_c,
                       const void* grad_out, int H, int W, int C, int dtype, int padding, double lambda,
                       void* grad_image, void* stream);

/* ---- Bilateral-grid appearance: per-image colour correction of a render, forward and backward (csrc/bilagrid.hip) ------
 * An addition: the reference has no appearance model.  image, out, grad_out, grad_image: contiguous (H, W, 3) arrays of
 * `dtype`, the rasterizer's layout.  grid, grad_grid: contiguous (12, L, Gy, Gx), the layout of published checkpoints;
 * coefficient 4c + j is row c, column j of a 3 x 4 affine colour matrix.  For the pixel at row y, column x, colour
 * p = (r, g, b):
 *   gx = (x + 0.5) / W (Gx - 1)    gy = (y + 0.5) / H (Gy - 1)
 *   lum = 0.299 r + 0.587 g + 0.114 b    gz = clamp(lum, 0, 1) (L - 1)
 *   A = trilinear interpolation of the 12 planes at (gz, gy, gx): the cell along an axis is min(floor(coord), size - 2),
 *       0 where the size is 1, and an axis of size 1 contributes its single plane with weight 1
 *   out = A[:, :3] p + A[:, 3]
 * which is torch's 5-D grid_sample(bilinear, padding_mode='border', align_corners=True) of the planes followed by the
 * affine.  A NaN luminance is clamped into bin 0 (that pixel's output may be NaN, no other's), +inf into the last.
 * ms_bilagrid_bwd, with g = grad_out and p1 = (r, g, b, 1):
 *   grad_grid[4c + j, z, yv, xv] = sum over pixels of w_z w_y w_x g_c p1_j,  w = max(0, 1 - |coord - vertex|) on the
 *       clamped coordinates; a vertex no pixel reaches receives exactly 0, and every element is written (the caller
 *       need not clear the array)
 *   grad_image = A[:, :3]^T g + [0 < lum < 1] (L - 1) (g^T (dA/dgz) p1) (0.299, 0.587, 0.114): the luminance guide is
 *       differentiated as grid_sample does, and is flat where it is clamped
 * grad_image NULL or grad_grid NULL skips that gradient (and its kernels).  grad_grid is a gather without atomics: a
 * workgroup sums one vertex's weights over a chunk of its footprint into tmp (double), a second kernel adds the chunks
 * in a fixed order: bit-reproducible.  (tmp, tmp_bytes): see Conventions (the size is the same whichever gradients
 * are asked for).  Neither call reads back to the host.
 * 1 <= L <= 16, 1 <= Gy, Gx <= 128, H W 3 < 2^31.
 * MS_ERR_BAD_ARG: null pointer, a size <= 0, both gradients NULL; MS_ERR_UNSUPPORTED: unknown dtype, sizes beyond the
 * limits; MS_ERR_TMP_TOO_SMALL. */
int ms_bilagrid_fwd(const void* image, const void* grid, int H, int W, int L, int Gy, int Gx, int dtype, void* out,
                    void* stream);
int ms_bilagrid_bwd(const void* image, const void* grid, const void* grad_out, int H, int W, int L, int Gy, int Gx,
                    int dtype, void* grad_image, void* grad_grid, void* tmp, size_t* tmp_bytes, void* stream);

/* ---- Geometry: per-gaussian normals, and the normal-consistency loss of a blended geometry image (csrc/geometry.hip) ----
 * An addition: the reference renders no normals.  float32 and float64; nothing reads back to the host; no atomics.
 *
 * ms_gaussian_normals_fwd: position (n, 3), log_scaling (n, 3), rotation (n, 4, xyzw, normalised on read),
 * camera_position 3 values in DEVICE memory.  normals (n, 3): column k of R(rotation / |rotation|), k the index of the
 * smallest log_scaling entry (a tie takes the lowest index), negated where normal . (position - camera_position) > 0
 * (exactly 0 keeps the sign).  code (n bytes) receives k | flipped << 2, which is all the backward needs of position,
 * log_scaling and camera_position.
 * ms_gaussian_normals_bwd: grad_rotation (n, 4) = d(normals . grad_normals) / d rotation through the unnormalised
 * quaternion, with k and the sign of `code` held constant.  There is no other gradient.
 *
 * ms_normal_consistency_fwd: accum is a contiguous (H, W, F) image whose channel depth_offset holds sum w z,
 * alpha_offset sum w, normal_offset .. normal_offset + 2 sum w n (camera frame); projection = (fx, fy, cx, cy) in DEVICE
 * memory; pixel centres at (x + 0.5, y + 0.5).  With d = depth_sum / alpha and P = d ((x + 0.5 - cx) / fx,
 * (y + 0.5 - cy) / fy, 1), for 1 <= x <= W - 2, 1 <= y <= H - 2:
 *   a = P(x + 1, y) - P(x - 1, y)    b = P(x, y + 1) - P(x, y - 1)    c = b x a   (a fronto-parallel plane: (0, 0, -1))
 *   n_d = c / |c| where |c|^2 >= MS_NORMAL_TINY, else 0;   n^ = normal_sum / |normal_sum| under the same rule
 *   out_loss[0] = sum of w (1 - n^ . n_d) / ((H - 2)(W - 2))
 * w = pixel_weight (H, W), or alpha where pixel_weight is NULL, where the pixel and its four neighbours all have
 * alpha >= alpha_min (> 0 required; d is evaluated nowhere else), and 0 elsewhere.  H < 3 or W < 3: exactly 0.
 * depth_normals: NULL or (H, W, 3), receives n_d (0 outside the interior and where w's indicator fails).  tmp holds one
 * double per workgroup, added in a fixed order by a second kernel: bit-reproducible.  (tmp, tmp_bytes): see
 * Conventions.
 * ms_normal_consistency_bwd: ONE launch; grad_accum (H, W, F) = grad_loss * d out_loss / d accum in the depth, alpha and
 * normal channels, exactly 0 in every other channel; every element is written.  w is a constant, a vector under
 * MS_NORMAL_TINY a constant 0, and there is no gradient for projection.  grad_loss is ONE value of `dtype` in DEVICE
 * memory.
 * MS_ERR_BAD_ARG: null pointer, a size <= 0, F < 5, channel offsets outside the image or overlapping, alpha_min <= 0;
 * MS_ERR_UNSUPPORTED: unknown dtype, H W F >= 2^31; MS_ERR_TMP_TOO_SMALL. */
#define MS_NORMAL_TINY 1e-30
int ms_gaussian_normals_fwd(const void* position, const void* log_scaling, const void* rotation,
                            const void* camera_position, int64_t n, int dtype, void* normals, void* code, void* stream);
int ms_gaussian_normals_bwd(const void* rotation, const void* code, const void* grad_normals, int64_t n, int dtype,
                            void* grad_rotation, void* stream);
int ms_normal_consistency_fwd(const void* accum, const void* pixel_weight, const void* projection, int H, int W, int F,
                              int depth_offset, int alpha_offset, int normal_offset, int dtype, double alpha_min,
                              void* tmp, size_t* tmp_bytes, void* out_loss, void* depth_normals, void* stream);
int ms_normal_consistency_bwd(const void* accum, const void* pixel_weight, const void* projection, const void* grad_loss,
                              int H, int W, int F, int depth_offset, int alpha_offset, int normal_offset, int dtype,
                              double alpha_min, void* grad_accum, void* stream);

/* ---- Scene transform: a similarity m = [[s R, t], [0, 1]] on a whole 3-D scene in one launch (csrc/scene_transform.hip) --
 * An addition: the reference's transform_rigid (data_types.py:91-102) moves position and rotation and leaves the SH
 * coefficients alone, so the view-dependent colour of a rotated scene points the old way.
 *   position'    = s R p + t
 *   log_scaling' = log_scaling + ln s
 *   rotation'    = q_R (x) q   (Hamilton product, xyzw; the row is NOT normalised — the kernels normalise on read — and a
 *                               zero row stays zero)
 *   feature'     : (n, f, (sh_degree + 1)^2); in the real basis of ms_sh_fwd, band l (coefficients l^2 .. (l + 1)^2 - 1)
 *                  of every (gaussian, channel) is replaced by M_l(R) c_l, where Y_l(R d) = M_l(R) Y_l(d) for every unit
 *                  d: the moved scene shows from the moved camera what the old one showed from the old.  Band 0 is
 *                  invariant.  alpha_logit and (n, C) colours do not change and are not arguments.
 * Each field is an (in, out) pair of (n, 3 | 3 | 4 | f K) arrays of `dtype`; a pair of NULLs skips the field, out == in
 * works in place, any other overlap is the caller's error.  sh_degree must be 1..3 and f >= 1 when a feature is given
 * (a degree-0 feature has nothing to rotate: pass NULLs).  Pointers need only the alignment of their element type: a
 * feature whose two bases are 16-byte aligned moves in 16-byte pieces, any other in 4-byte pieces.
 * transform_host: MS_SCENE_XFORM_VALUES doubles in HOST memory, read during the call and passed on as kernel arguments
 * (no device buffer, no host read of device memory, no allocation, no synchronisation: the call can be captured into a
 * graph): [s R | t] row-major 3x4, ln s, q_R (xyzw), then M_1 (3x3), M_2 (5x5), M_3 (7x7) row-major (the matrices
 * above sh_degree are not read).  The geometry is evaluated in double and rounded once; the matrices are rounded to
 * `dtype` and applied with FMAs.  A workgroup takes MS_SCENE_XFORM_ROWS consecutive rows.
 * n == 0: returns 0 without a launch.  MS_ERR_BAD_ARG: n < 0 or >= 2^31, sh_degree outside 1..3 or f < 1 with a feature,
 * one pointer of a pair NULL and the other not, unknown dtype, NULL transform_host, a misaligned pointer. */
#define MS_SCENE_XFORM_ROWS 256
enum {
  MS_SCENE_XFORM_SRT = 0,      /* 12 values */
  MS_SCENE_XFORM_LN_S = 12,
  MS_SCENE_XFORM_QUAT = 13,    /* 4 values */
  MS_SCENE_XFORM_M1 = 17,      /* 9 values */
  MS_SCENE_XFORM_M2 = 26,      /* 25 values */
  MS_SCENE_XFORM_M3 = 51,      /* 49 values */
  MS_SCENE_XFORM_VALUES = 100
};
int ms_scene_transform(const void* position, void* out_position, const void* log_scaling, void* out_log_scaling,
                       const void* rotation, void* out_rotation, const void* feature, void* out_feature,
                       int64_t n, int f, int sh_degree, int dtype, const double* transform_host, void* stream);

/* ---- Camera-set coverage: which cameras see each gaussian, in one launch (csrc/camera_coverage.hip) -------------------
 * An addition: neither the reference nor ms_project_fwd looks at a scene through more than one camera at a time, so
 * "which gaussians does no training view render", "by how many views is each seen" and "at what sampling rate" cost a
 * loop of projections, one host read of the visible count and one index tensor per camera.
 * One lane per gaussian loops over all cameras.  "In view" is bit for bit the decision ms_project_fwd takes for that
 * camera with its own image size and clip planes and this call's blur_cov, clamp_margin and alpha_threshold — the
 * alpha-below-threshold NaN path and a zero or non-finite quaternion included, both culled.
 *   out_count     (n) int32: number of cameras that have gaussian i in view
 *   out_max_rate  (n) `dtype`: max over those cameras of max(fx, fy) / z, one division in `dtype`, z the camera-space
 *                 depth ms_project_fwd writes; 0 where out_count is 0.  The sampling rate Mip-Splatting's 3-D filter
 *                 is built from.
 *   out_min_depth (n) `dtype`: min over those cameras of z; +inf where out_count is 0
 *   out_mask      NULL, or (ceil(num_cameras / 32), n) uint32, WORD-major: bit c % 32 of out_mask[(c / 32) * n + i] is
 *                 set exactly when camera c has gaussian i in view; unused high bits of the last word are zero.
 * cameras: a DEVICE array (num_cameras, MS_COVERAGE_CAMERA_VALUES) of `dtype`, per camera: rows 0..2 of T_camera_world
 * row-major (12 values), fx, fy, cx, cy, near, far, width, height.  Every lane reads it wave-uniformly (scalar loads).
 * position (n, 3), log_scaling (n, 3), rotation (n, 4), alpha_logit (n) as for ms_project_fwd; dtype MS_F32 or MS_F64.
 * No atomics: the outputs are bitwise reproducible.  No allocation, no synchronisation, no host read of device memory:
 * the call can be captured into a graph.  n == 0: returns 0 without a launch.  Every argument is checked before the
 * launch; MS_ERR_BAD_ARG: n < 0 or >= 2^31, num_cameras outside 1..MS_COVERAGE_MAX_CAMERAS, unknown dtype, a pointer not
 * aligned to its element type, a NULL pointer other than out_mask with n > 0.
 * Measured on an MI355X, 6 M random gaussians, float32, masks included: 16 / 64 / 256 cameras in 0.80 / 2.99 / 11.8 ms
 * (130 G pairs per second, the same without masks), against 5.0 / 19.7 / 78.8 ms for the loop of ms_project_fwd, scan, host
 * read, gather and torch scatters it replaces: 6.2 - 6.7 x (profiles/camera_coverage.txt). */
#define MS_COVERAGE_CAMERA_VALUES 20
#define MS_COVERAGE_MAX_CAMERAS 65535
int ms_camera_coverage(const void* position, const void* log_scaling, const void* rotation, const void* alpha_logit,
                       const void* cameras, int num_cameras, double blur_cov, double clamp_margin,
                       double alpha_threshold, int64_t n, int32_t* out_count, void* out_max_rate, void* out_min_depth,
                       uint32_t* out_mask /* may be NULL */, int dtype, void* stream);

/* ---- Fixed-budget densification: relocate dead gaussians, perturb positions (csrc/relocate.hip) -----------------------
 * An addition with no reference counterpart: the strategy of 3DGS-MCMC (Kheradmand et al., "3D Gaussian Splatting as
 * Markov Chain Monte Carlo", NeurIPS 2024).  The row count never changes and every array keeps its storage; no call
 * allocates, synchronises or reads device memory from the host, so the whole step can be captured into a graph.
 * All float arrays are float32; n < 2^30.  The calls of one step, in order, on one stream:
 *
 * ms_relocate_weights: row i is dead iff !(alpha_logit[i] > threshold) (NaN is dead); threshold is
 *   float32(logit(min_opacity)), computed by the caller in double.  weights[i] (int64) = 0 for a dead row, else
 *   max(1, llrint(sigmoid(alpha_logit[i]) 2^24)) evaluated in double.  Also clears count (n int32) and counts (3 int64)
 *   for the calls below.
 * The caller then forms cdf = the inclusive int64 sum of weights (exact, whatever the order of the additions).
 * ms_relocate_draw: random is n 64-bit words read as unsigned.  With total = cdf[n - 1] > 0 a dead row i takes
 *   target = (random[i] * total) >> 64, src[i] = the first j with cdf[j] > target (a live row) and adds 1 to count[j];
 *   a live row gets src[i] = i.  With total == 0 (every row dead) every row gets src[i] = i and nothing will move.
 *   counts[0] = number of dead rows, counts[2] = total.
 * ms_relocate_fresh: for every row j with count[j] > 0, in double from the float32 inputs, rounded once:
 *     ratio = min(count[j] + 1, MS_RELOCATE_MAX_RATIO)    o = sigmoid(alpha_logit[j])    o' = 1 - (1 - o)^(1 / ratio)
 *     denom = sum_{i = 1 .. ratio} sum_{k = 0 .. i - 1} C(i - 1, k) (-1)^k o'^(k + 1) / sqrt(k + 1)    coeff = o / denom
 *     fresh_opacity[j] = logit(clamp(o', min_opacity, 1 - 1e-7))
 *     fresh_scale[j, d] = log_scaling[j, d] + ln(coeff)      for d < scale_dims (1 .. 16)
 *   binomials: DEVICE array of MS_RELOCATE_MAX_RATIO^2 doubles, row-major, [m][k] = C(m, k) (0 for k > m).  Rows that were
 *   not drawn are not written.  counts[1] = number of drawn rows.
 * ms_relocate_move: every array of the scene in ONE launch, IN PLACE.  A row is touched if it is dead and moves
 *   (src[i] != i) or live and drawn (count[i] > 0); an untouched row is neither read nor written.  By role:
 *     MS_RELOCATE_COPY          a moved row takes row src[i] of the same array; a drawn row keeps its own
 *     MS_RELOCATE_ZERO_TOUCHED  moved and drawn rows become zero (optimiser moments)
 *     MS_RELOCATE_INHERIT       as MS_RELOCATE_COPY (state that follows the gaussian, e.g. a running visibility)
 *     MS_RELOCATE_OPACITY / MS_RELOCATE_SCALE   moved and drawn rows take row src[i] of `fresh`, a side buffer with the
 *                               array's row layout written by ms_relocate_fresh: a source's new values are never read
 *                               from the array that is being written
 *   Sources are live and destinations dead, so the copies of one array never overlap.  Rows move as 16-byte pieces when
 *   row_bytes % 16 == 0 and the bases are 16-byte aligned, as 4-byte pieces otherwise; row_bytes must be a positive
 *   multiple of 4 (at most 1 MiB).  Every descriptor is checked before the first launch.  `arrays` is a HOST array.
 * MS_ERR_BAD_ARG: n outside [0, 2^30), a NULL or misaligned pointer, scale_dims outside 1..16, min_opacity outside
 * (0, 1 - 1e-7), NaN threshold, an unknown role, fresh == data; MS_ERR_ABI: a descriptor of another size. */
#define MS_RELOCATE_MAX_RATIO 51
enum { MS_RELOCATE_COPY = 0, MS_RELOCATE_ZERO_TOUCHED = 1, MS_RELOCATE_INHERIT = 2, MS_RELOCATE_OPACITY = 3,
       MS_RELOCATE_SCALE = 4 };
typedef struct ms_relocate_array {
  uint32_t struct_size;            /* sizeof(ms_relocate_array) */
  int32_t role;                    /* MS_RELOCATE_* */
  void* data;                      /* (n, row_bytes), modified in place */
  const void* fresh;               /* (n, row_bytes) side buffer of the OPACITY / SCALE roles, ignored otherwise */
  int64_t row_bytes;
} ms_relocate_array;
int ms_relocate_weights(const float* alpha_logit, int64_t n, float threshold, int64_t* weights, int32_t* count,
                        int64_t* counts, void* stream);
int ms_relocate_draw(const int64_t* weights, const int64_t* cdf, const uint64_t* random, int64_t n, int32_t* src,
                     int32_t* count, int64_t* counts, void* stream);
int ms_relocate_fresh(const float* alpha_logit, const float* log_scaling, int scale_dims, const int32_t* count, int64_t n,
                      double min_opacity, const double* binomials, float* fresh_opacity, float* fresh_scale,
                      int64_t* counts, void* stream);
int ms_relocate_move(const ms_relocate_array* arrays, int num_arrays, const int32_t* src, const int32_t* count, int64_t n,
                     void* stream);

/* ms_perturb_positions: the exploration noise of the same paper, one lane per gaussian, in place on position (n, 3):
 *   position += step g(o) Sigma z      Sigma = R diag(exp(2 log_scaling)) R^T      o = sigmoid(alpha_logit)
 *   g(o) = 1 / (1 + exp(-k ((1 - o) - x0)))          (the paper: k = 100, x0 = 0.995)
 * R is the rotation of the xyzw quaternion normalised as in the projection; z (n, 3) is drawn by the caller.  step g is
 * evaluated in double (k amplifies a float32 rounding of 1 - o a hundredfold, and g of an opaque gaussian lies below the
 * float32 normal range), Sigma z in float32, their product is rounded to float32 once.  A row whose
 * step g(o) is exactly zero, whose offset is zero, or whose quaternion is zero or not finite keeps its position bit
 * for bit.  With position, log_scaling, rotation and z 16-byte aligned every access is 16 bytes wide, else 4.
 * MS_ERR_BAD_ARG: n outside [0, 2^31), a NULL or misaligned pointer, a NaN step, k or x0. */
int ms_perturb_positions(float* position, const float* log_scaling, const float* rotation, const float* alpha_logit,
                         const float* z, int64_t n, float step, double k, double x0, void* stream);

/* ---- k-means over (N, D) float32 rows: the two halves of a Lloyd iteration (no reference counterpart) ----
 * 1 <= d <= MS_KMEANS_MAX_D, 1 <= k <= MS_KMEANS_MAX_K, 0 <= n < 2^31 - 1024.  Both calls: (tmp, tmp_bytes) as in
 * Conventions, sized by (n, d, k); no host read, allocation, synchronisation or atomic, so they capture into a graph and two
 * runs are bitwise equal.  MS_ERR_BAD_ARG names the argument.
 *
 * ms_kmeans_assign: out_index[i] = argmin_j s(i, j), s(i, j) = ||c_j||^2 - 2 x_i . c_j evaluated on the exact
 * f32-input MFMA as the fmaf chain that starts at ||c_j||^2 (a float64 sum rounded once) and adds -2 x_ik c_jk for
 * k = 0..d-1 in order; the lowest index wins a tie.  out_dist2[i] (may be NULL) = max(s_best + ||x_i||^2, 0) with
 * ||x_i||^2 a float64 sum rounded once.  A workgroup stages MS_KMEANS_CHUNK codes per pass.  x and codebook must be
 * finite (a NaN or infinity gives an unspecified index in 0..k-1, no stray access).  n == 0 launches nothing.
 *
 * ms_kmeans_update: codebook[j] = sum_i w_i x_i / sum_i w_i over index[i] == j, in place; weights (N,) >= 0 or NULL
 * (all 1).  float64 accumulation in an order fixed by (n, index): pairs sorted by code with ms_radix_sort_pairs, runs
 * cut into MS_KMEANS_UPDATE_CHUNK entries, chunks combined in list order.  A code with no member or zero weight keeps
 * its row bit for bit.  out_counts (k,) = members per code; out_weight_sums (k,) float64 may be NULL.  An index outside
 * 0..k-1 is clamped (wrong result, no stray access). */
#define MS_KMEANS_MAX_D 64
#define MS_KMEANS_MAX_K 65536
#define MS_KMEANS_CHUNK 128
#define MS_KMEANS_UPDATE_CHUNK 1024
int ms_kmeans_assign(const float* x, int64_t n, int d, const float* codebook, int k, int32_t* out_index,
                     float* out_dist2 /* may be NULL */, void* tmp, size_t* tmp_bytes, void* stream);
int ms_kmeans_update(const float* x, const int32_t* index, const float* weights /* may be NULL */, int64_t n, int d,
                     int k, float* codebook, int32_t* out_counts, double* out_weight_sums /* may be NULL */, void* tmp,
                     size_t* tmp_bytes, void* stream);

/* ---- colours of a vector-quantised scene from its stored form (no reference counterpart: an addition) ----
 * colour_c(i) = clamp(0.5 + Y_0 dc[i, c] + sum_{d >= 1} Y_d(dir_i) codebook[index[i], c, d - 1], 0, 1) with
 * dir_i = (positions[i] - cam_pos) / |.|: what ms_sh_fwd gives for the decoded rows cat(dc, codebook[index]), without
 * the decoded (n, 3, D) tensor or its gradient.  float32, 3 channels, sh_degree 1..3 (the stored degree), 1 <= k <=
 * 65 536, 0 <= n < 2^31 - 512.  dc (n, 3), index (n,) int32, codebook (k, 3, M) with M = (sh_degree + 1)^2 - 1,
 * positions (n, 3), cam_pos (3,), out (n, 3).  An index outside 0..k-1 is clamped (wrong result, no stray access).
 * Neither call reads on the host, allocates or synchronises: both capture into a graph.
 *
 * ms_sh_coded_fwd: one lane per gaussian in storage order; products summed for d = 0 .. D - 1, then + 0.5, then the
 * clamp.  The code row is gathered as stored (4-byte aligned).  n == 0 launches nothing.
 *
 * ms_sh_coded_bwd: per channel g = g_out where 0 < out < 1 (out is the clamped colour the forward wrote), else 0.
 *   g_dc[i, c] = g Y_0                                              dense, may be NULL
 *   g_codebook[j, c, d - 1] = sum over index[i] == j of g_c(i) Y_d(dir_i)      every row written, may be NULL
 * The codebook sum has no atomics and an order fixed by the plan, which the caller derives from index alone: the
 * gaussians listed by code, stably (storage order inside a code); rank (n,) is the place of each gaussian in that list;
 * the run of a code is cut into chunks of MS_SH_CODED_CHUNK entries, chunk_begin (num_chunks,) is the first entry of each
 * chunk in list order (a chunk ends where the next begins), chunk_off (k + 1,) the first chunk of each code.  A
 * storage-order pass writes (g, dir) of every gaussian into its place of the list, a workgroup sums the products
 * (double)g (double)Y of one chunk, a wave adds the chunks of one code in list order and rounds to float32 once: two
 * runs are bitwise equal.  Entries of the plan are clamped to their ranges.  With g_codebook == NULL only out and g_out
 * are read.  (tmp, tmp_bytes) as in Conventions, sized by (n, num_chunks, sh_degree): the chunk sums and 24 bytes per
 * gaussian.  MS_ERR_BAD_ARG names the argument. */
#define MS_SH_CODED_CHUNK 512
int ms_sh_coded_fwd(const float* dc, const int32_t* index, const float* codebook, const float* positions,
                    const float* cam_pos, int64_t n, int k, int sh_degree, float* out, void* stream);
int ms_sh_coded_bwd(const float* positions, const float* cam_pos, const float* out, const float* g_out,
                    const int32_t* rank, const int32_t* chunk_begin, const int32_t* chunk_off, int64_t num_chunks, int64_t n,
                    int k, int sh_degree, float* g_dc /* may be NULL */, float* g_codebook /* may be NULL */, void* tmp,
                    size_t* tmp_bytes, void* stream);

/* ---- TSDF fusion and marching tetrahedra: depth frames -> volume -> triangle mesh (csrc/tsdf.hip; an addition) ---------
 * The volume: tsdf and weight (nz, ny, nx) float32, colour (nz, ny, nx, 3) float32 or NULL, x fastest; sample (i, j, k)
 * sits at origin + voxel_size (i, j, k), evaluated in float32 as o + v * (float)i per axis.  origin_host is a HOST array
 * of 3 doubles; it, voxel_size, truncation, max_weight and min_weight are rounded to float32 once.  Every dim >= 1 and
 * nx ny nz <= MS_TSDF_MAX_SAMPLES = 2^27: 7 possible vertices and 12 possible triangles per cell then fit the int32
 * scans.  No call allocates, synchronises, reads device memory on the host or uses an atomic: each captures into a graph
 * and two runs are bitwise equal.  MS_ERR_BAD_ARG (before any launch): dims outside the limits, voxel_size or truncation
 * not > 0, max_weight not > 0, NaN min_weight, num_cameras outside 1..MS_COVERAGE_MAX_CAMERAS, an empty image, a NULL or
 * misaligned pointer (16 bytes for tsdf, weight and colour of ms_tsdf_integrate, 4 for the rest), colour without image or
 * image without colour.
 *
 * ms_tsdf_integrate: ONE launch for num_cameras frames.  depth (C, H, W) camera-z depth, 0 where uncovered;
 * pixel_weight (C, H, W) or NULL (all 1); image (C, H, W, 3), given exactly when colour is; cameras (C, 20) float32 DEVICE
 * rows of MS_COVERAGE_CAMERA_VALUES values as for ms_camera_coverage (the width and height of the rows are not read: all
 * frames share the call's).  For every sample p and c = 0 .. C - 1 in that order, float32, no FMA contraction, sums left
 * to right:
 *   (x, y, z) = T_camera_world[c][:3] (p, 1)                                       skip unless near <= z <= far
 *   u = fx x / z + cx, v = fy y / z + cy, ix = floor(u), iy = floor(v)             skip unless 0 <= ix < W, 0 <= iy < H
 *   d = depth[c, iy, ix]                                                           skip unless d > 0 and finite
 *   w = pixel_weight[c, iy, ix] or 1                                               skip unless w > 0
 *   s = d - z                                                                      skip if s < -truncation
 *   t = min(1, s / truncation);  W' = weight + w;  tsdf = (weight tsdf + w t) / W';  colour likewise with
 *   image[c, iy, ix];  weight = min(W', max_weight)          (max_weight = +infinity: no clamp)
 * A skipped sample keeps the bits of its three fields.  A lane owns MS_TSDF_RUN consecutive samples and keeps them in
 * registers over the camera loop: the volume is read and written at most once per call, so C frames in one call equal C
 * calls in the same order bit for bit.  Each wave tests the box of its samples against every camera's clip range and
 * frustum (MS_TSDF_CAMERA_CHUNK cameras per ballot; conservative) and touches the volume only if a camera is left.
 *
 * ms_tsdf_classify / ms_tsdf_emit: marching tetrahedra on the Kuhn split of each cell into the six corner paths
 * (0,0,0) -> (1,1,1), one per axis permutation, in lexicographic order of the permutation.  A sample is valid iff
 * weight > 0 and weight >= min_weight, inside iff tsdf < 0; a tetrahedron emits only when its four corners are valid.
 * A mesh vertex lies on a grid edge o -> o + d with both ends valid and of different sign, owned by o, edge types 0..6 =
 * d in the order 100 010 001 110 101 011 111 (x y z bits), at p_o + l (p_b - p_o), l = t_o / (t_o - t_b); colour with the
 * same l.  Vertices are ordered by (linear index of o, type), triangles by (linear index of the cell's lower corner,
 * tetrahedron, triangle); (b - a) x (c - a) points to the positive side.  Per tetrahedron with path corners 0..3: one
 * corner a apart from b < c < d gives (ab, ac, ad); inside a < b and outside c < d give (ac, bd, bc) then (ac, ad, bd);
 * the last two of a triple are swapped as orientation demands (csrc/tsdf.hip).
 *   classify: word[o] = mask (7 bits) | triangles of cell o << 8; vertex_count[o] = popcount(mask), triangle_count[o]:
 *             the inputs of two ms_exclusive_scan_i32 (which may run in place: out == in needs n + 1 entries).
 *   emit:     vertices of o at vertex_scan[o] + rank, triangles of cell o from triangle_scan[o]; a triangle finds a
 *             vertex as vertex_scan[owner] + popcount(word[owner] & ((1 << type) - 1)).  out_vertices (V, 3),
 *             out_faces (T, 3) int32, out_colours (V, 3) or NULL.  The caller sizes them from the scans' totals — the
 *             one host read of an extraction — and skips the call when V = 0.
 * Scratch: 12 bytes per sample (word and the two scans, n + 1 entries each) + the scan's tmp. */
#define MS_TSDF_MAX_SAMPLES (1 << 27)
#define MS_TSDF_RUN 4
#define MS_TSDF_CAMERA_CHUNK 64
int ms_tsdf_integrate(float* tsdf, float* weight, float* colour /* may be NULL */, int nx, int ny, int nz,
                      const double* origin_host, double voxel_size, double truncation, double max_weight,
                      const float* depth, const float* pixel_weight /* may be NULL */, const float* image /* may be NULL */,
                      const float* cameras, int num_cameras, int width, int height, void* stream);
int ms_tsdf_classify(const float* tsdf, const float* weight, int nx, int ny, int nz, double min_weight, int32_t* word,
                     int32_t* vertex_count, int32_t* triangle_count, void* stream);
int ms_tsdf_emit(const float* tsdf, const float* weight, const float* colour /* may be NULL */, int nx, int ny, int nz,
                 const double* origin_host, double voxel_size, double min_weight, const int32_t* word,
                 const int32_t* vertex_scan, const int32_t* triangle_scan, float* out_vertices, int32_t* out_faces,
                 float* out_colours /* may be NULL */, void* stream);

/* ---- Mesh clean-up: connected components, face selection, vertex normals (csrc/mesh.hip; an addition) -----------------
 * A mesh is vertices (V, 3) float32 and faces (T, 3) int32, contiguous; 0 <= V <= MS_MESH_MAX_VERTICES and
 * 0 <= 3 T <= MS_MESH_MAX_CORNERS (MS_ERR_BAD_ARG before any launch otherwise).  T = 0, V = 0, degenerate faces (a == b),
 * duplicate faces and vertices no face references are all legal.  Faces are connected through shared vertex indices only.
 * No call allocates, synchronises or reads device memory on the host; two runs of any call give bitwise-equal outputs.
 * Every (tmp, tmp_bytes) follows Conventions, and tmp must be aligned to 256 bytes (MS_ERR_BAD_ARG otherwise).
 *
 * LABEL RULE (ms_mesh_components).  Two vertices belong to one component iff a chain of faces links them.  Labels are
 * dense, 0 .. K - 1, ordered by the smallest vertex index of the component; a vertex no face references gets -1, belongs
 * to no component and is not counted; face_label[f] is the label of its corners.  The rule makes the labels independent
 * of launch order and of any permutation of the face list.  Construction: lock-free union-find (the larger root is
 * hooked under the smaller with a compare-and-swap, retried from the returned parent; every loop is bounded: walks by V,
 * retries by a fixed cap), a flatten pass, one exclusive scan of the root flags, labels by gather.  head (2 int32 on the
 * DEVICE, for the caller's one host read) receives (K, status): status is 0 or a sum of MS_MESH_BAD_INDEX (a face index
 * outside 0 .. V - 1: found on the device, nothing is read or written through it; its face_label is -1) and
 * MS_MESH_GAVE_UP (a lane exhausted its retries: the labels are not to be used).  head is poisoned to (-1, -1) first.
 * ms_mesh_component_counts: vertex_count and face_count (K,) int32, zero-filled by the call; equal labels are combined
 * inside a wave before one integer add.
 * ms_mesh_component_filter: face_mask[f] (uint8 0 / 1) = the component of f has face_count >= min_faces (>= 1) and, when
 * keep_largest > 0, is among the keep_largest largest of those by face count, a tie going to the lower label
 * (keep_largest == 0: no such limit).  A face with label -1 is dropped.
 *
 * SELECTION ORDER (ms_mesh_select_plan / ms_mesh_select_gather).  The faces with face_mask != 0 are kept, in input order;
 * the vertices a kept face references are kept, in input order (stable); a kept row of vertices, colours or normals is
 * the input row bit for bit; indices are remapped.  plan: vertex_scan (V + 1) and face_scan (T + 1) int32 = exclusive
 * scans of the keep flags, head (3 int32, device) = (V', T', status) with MS_MESH_BAD_INDEX when a KEPT face holds an
 * index outside 0 .. V - 1 (the caller must then not gather).  The caller sizes the outputs from head: the one host read.
 *
 * NORMAL FORMULA (ms_mesh_vertex_normals).  s(v) = sum over the corners (f, k) with faces[f][k] == v, in ascending corner
 * index 3 f + k, of (b - a) x (c - a) with (a, b, c) the positions of face f: the area-weighted normal, oriented as the
 * faces are (outward for ms_tsdf_emit).  Differences, products and the running sum are FLOAT64 operations on the float32
 * positions, in that order, without FMA contraction; out_sums (V, 3) is s rounded to float32 once, out_normals (V, 3) is
 * s / |s| (float64 division by the float64 length) rounded to float32 once; either may be NULL.  A vertex with |s| = 0
 * (or not finite), or that no face references, gets the normal (0, 0, 0), never a NaN.  A face with an index outside
 * 0 .. V - 1 contributes nothing (this call reports no status: it has no host read and captures into a graph).  No float
 * atomics: the incidence comes from a stable ms_radix_sort_pairs of the 3 T (vertex, corner) pairs and ms_find_ranges. */
#define MS_MESH_MAX_VERTICES 2147483647
#define MS_MESH_MAX_CORNERS 2147483647
#define MS_MESH_BAD_INDEX 1
#define MS_MESH_GAVE_UP 2
int ms_mesh_components(const int32_t* faces, int64_t num_vertices, int64_t num_faces, int32_t* vertex_label,
                       int32_t* face_label, int32_t* head, void* tmp, size_t* tmp_bytes, void* stream);
int ms_mesh_component_counts(const int32_t* vertex_label, int64_t num_vertices, const int32_t* face_label, int64_t num_faces,
                             int64_t num_components, int32_t* vertex_count, int32_t* face_count, void* stream);
int ms_mesh_component_filter(const int32_t* face_count, int64_t num_components, int64_t min_faces, int64_t keep_largest,
                             const int32_t* face_label, int64_t num_faces, uint8_t* face_mask, void* tmp, size_t* tmp_bytes,
                             void* stream);
int ms_mesh_select_plan(const int32_t* faces, const uint8_t* face_mask, int64_t num_vertices, int64_t num_faces,
                        int32_t* vertex_scan, int32_t* face_scan, int32_t* head, void* tmp, size_t* tmp_bytes, void* stream);
int ms_mesh_select_gather(const float* vertices, const float* colours /* may be NULL */, const float* normals /* may be NULL */,
                          const int32_t* faces, const uint8_t* face_mask, int64_t num_vertices, int64_t num_faces,
                          const int32_t* vertex_scan, const int32_t* face_scan, float* out_vertices, float* out_colours,
                          float* out_normals, int32_t* out_faces, void* stream);
int ms_mesh_vertex_normals(const float* vertices, const int32_t* faces, int64_t num_vertices, int64_t num_faces,
                           float* out_sums /* may be NULL */, float* out_normals /* may be NULL */, void* tmp,
                           size_t* tmp_bytes, void* stream);

/* ---- Mesh simplification: vertex clustering with a quadric-error representative (csrc/mesh_simplify.hip; an addition) ---
 * Rossignac & Borrel's clustering on a uniform grid with Lindstrom's (SIGGRAPH 2000) quadric placement per cell: one
 * output vertex per occupied cell, the faces whose three corners fall into three different cells.  A sort, two scans and
 * a per-cluster reduction; no float atomics; two runs give bitwise-equal outputs.  Meshes are as above.  NO entry point
 * here takes a scratch block: every array is the caller's, and the caller runs ms_radix_sort_pairs (stable),
 * ms_exclusive_scan_i32, ms_find_ranges and ms_mesh_select_plan / ms_mesh_select_gather between the calls, in the order
 * the functions are declared below.  Output sizes depend on the data (two host reads: (K, status), then the selection's),
 * so the sequence does not capture into a graph.
 *
 * CELL RULE.  cell(p) = floor((p - origin) / cell_size) per axis IN FLOAT32: one IEEE subtraction, one correctly rounded
 * division, one floor (numpy float32 reproduces it bit for bit).  origin is 3 float32 ON THE DEVICE, cell_size a finite
 * positive float32.  A cell index lies in 0 .. MS_MESH_SIMPLIFY_MAX_CELL = 2^21 - 1 per axis; the key of a cell is
 * z << 42 | y << 21 | x.  Only vertices a face references are clustered: the others get the key 2^64 - 1, which sorts
 * last, and cluster -1.  status (1 int32, device) receives 0 or a sum of MS_MESH_BAD_INDEX (a face index outside
 * 0 .. V - 1; nothing is read or written through it), MS_MESH_NOT_FINITE (a referenced vertex with a NaN or an infinity)
 * and MS_MESH_CELL_RANGE (a referenced, finite vertex whose cell index leaves the range, or is no number because origin
 * is none); the caller must stop at a non-zero status.  head (2 int32, device) is poisoned to (-1, -1) by
 * ms_mesh_simplify_keys and receives (K, status) from ms_mesh_simplify_clusters.
 *
 * ORDER RULE.  Clusters — and so output vertices — are in ascending key order; the members of a cluster are in ascending
 * vertex index (the sort is stable); output faces keep the input order.
 *
 * FACE RULE.  A face is rewritten to its corners' clusters; it is dropped when two of them are equal, otherwise rotated
 * so that its smallest index comes first (the orientation stays).  Of faces with the same rotated triple the one with the
 * lowest input index survives; a pair with opposite orientation is not a duplicate.  Construction: a stable sort of
 * (third index, face), ms_mesh_simplify_pair_keys in that order, a stable sort of (first << shift | second, face) with
 * 2^shift > K - 1: equal triples are then adjacent in ascending face index, and ms_mesh_simplify_dedup clears keep[f] of a
 * face whose triple equals its predecessor's.  new_faces holds (0, 0, 0) for a dropped face.  Clusters left without a
 * face go in the selection's compaction (SELECTION ORDER), and ms_mesh_simplify_map composes the two maps:
 * vertex_map[v] = the output vertex of v, -1 for a vertex no face references or whose cluster lost all its faces.
 *
 * PLACEMENT RULE (ms_mesh_simplify_place).  xm = the float64 mean of the cluster's member positions.
 * MS_MESH_SIMPLIFY_MEAN places the vertex at xm, rounded to float32 once.  MS_MESH_SIMPLIFY_QUADRIC: over every corner
 * (f, k) whose vertex is in the cluster (a face counts once per such corner), with (a, b, c) the positions of face f,
 * m = (b - a) x (c - a) and d = -m . (a - xm) in float64 on the float32 positions: A = sum m m^T, r = sum d m, and
 * x = xm - (A + lambda I)^-1 r with lambda = regularisation trace(A) / 3 — the minimiser of the summed squared
 * area-weighted plane distances plus a pull of relative weight `regularisation` towards the mean; a closed-form 3 x 3
 * symmetric positive definite solve (adjugate over determinant) of condition number <= 1 + 3 / regularisation.  x is
 * rounded to float32 once and accepted only if cell(x), by the CELL RULE, is the cluster's own cell; otherwise, or when
 * trace(A) == 0 or x is not finite, the vertex is xm rounded once, under the same test; failing that too it is the member
 * with the lowest index, bit for bit.  INVARIANT: every output vertex lies in its own cluster's cell under the CELL RULE,
 * so simplifying the result again with the same origin and cell_size returns the same faces.  Summation order: 16 lanes
 * share a cluster, lane j adds the entries j, j + 16, .. of the run (members in ascending vertex index, corners in
 * ascending corner index 3 f + k) and the 16 partials meet in a fixed butterfly (1, 2, 4, 8 lanes apart): the order
 * depends on the run's length alone.  out_colours (when colours is given) = the float64 mean of the members' colours,
 * rounded once; normals are not carried.  out_choice (K uint8, may be NULL) = which of the three the cluster took. */
#define MS_MESH_NOT_FINITE 4
#define MS_MESH_CELL_RANGE 8
#define MS_MESH_SIMPLIFY_MAX_CELL 2097151
#define MS_MESH_SIMPLIFY_QUADRIC 0
#define MS_MESH_SIMPLIFY_MEAN 1
#define MS_MESH_SIMPLIFY_MEMBER 2
/* origin (3 float32, device) = the smallest FINITE coordinate of all V vertices per axis — the default origin: the lowest
 * vertex then falls into cell 0; +infinity for an axis without a finite value, (0, 0, 0) for V = 0.  -0 counts as below
 * +0, so the bits of the result are defined as well.  Integer atomics on the float's bits, chosen by the sign bit (a
 * minimum in a total order does not depend on the order of its operands). */
int ms_mesh_simplify_origin(const float* vertices, int64_t num_vertices, float* origin, void* stream);
/* referenced (V) int32 is scratch of the call; keys (V) u64 and values (V) = 0 .. V - 1 are the pairs to sort on bits 0 .. 64 */
int ms_mesh_simplify_keys(const float* vertices, const int32_t* faces, int64_t num_vertices, int64_t num_faces,
                          const float* origin, float cell_size, int32_t* referenced, uint64_t* keys, int32_t* values,
                          int32_t* status, int32_t* head, void* stream);
/* head_flag (V + 1) int32: [i] = the sorted key i opens a cluster; the caller scans it in place ([V] = K) */
int ms_mesh_simplify_heads(const uint64_t* sorted_keys, int64_t num_vertices, int32_t* head_flag, void* stream);
/* vertex_cluster (V) int32; member_begin (V + 1) int32, of which [0 .. K] are written: cluster c owns the sorted entries
 * member_begin[c] .. member_begin[c + 1] - 1 */
int ms_mesh_simplify_clusters(const uint64_t* sorted_keys, const int32_t* sorted_vertices, const int32_t* head_scan,
                              int64_t num_vertices, int32_t* vertex_cluster, int32_t* member_begin, const int32_t* status,
                              int32_t* head, void* stream);
/* keys, values (3 T): (cluster, corner) pairs, to sort on the low bits that hold K; then ms_find_ranges over K clusters */
int ms_mesh_simplify_corner_keys(const int32_t* faces, int64_t num_vertices, int64_t num_faces, const int32_t* vertex_cluster,
                                 int64_t num_clusters, uint32_t* keys, int32_t* values, void* stream);
/* corner_ranges (K, 2) and sorted_corners (3 T) may be NULL with MS_MESH_SIMPLIFY_MEAN */
int ms_mesh_simplify_place(const float* vertices, const float* colours /* may be NULL */, const int32_t* faces,
                           int64_t num_vertices, int64_t num_faces, const float* origin, float cell_size,
                           double regularisation, int placement, const uint64_t* sorted_keys, const int32_t* sorted_vertices,
                           const int32_t* member_begin, int64_t num_clusters, const int32_t* corner_ranges,
                           const int32_t* sorted_corners, float* out_vertices, float* out_colours, uint8_t* out_choice,
                           void* stream);
/* new_faces (T, 3), third_keys (T), values (T) = 0 .. T - 1, keep (T) uint8 */
int ms_mesh_simplify_faces(const int32_t* faces, int64_t num_vertices, int64_t num_faces, const int32_t* vertex_cluster,
                           int64_t num_clusters, int32_t* new_faces, uint32_t* third_keys, int32_t* values, uint8_t* keep,
                           void* stream);
int ms_mesh_simplify_pair_keys(const int32_t* new_faces, const int32_t* order, int64_t num_faces, int shift,
                               uint64_t* pair_keys, void* stream);
int ms_mesh_simplify_dedup(const int32_t* new_faces, const int32_t* order, int64_t num_faces, uint8_t* keep, void* stream);
/* cluster_scan (K + 1): vertex_scan of ms_mesh_select_plan over the K clusters */
int ms_mesh_simplify_map(const int32_t* vertex_cluster, int64_t num_vertices, const int32_t* cluster_scan,
                         int64_t num_clusters, int32_t* vertex_map, void* stream);

/* ---- Surface samples of a mesh (csrc/mesh_sample.hip; an addition: what a mesh is scored through) -----------------------
 * Uniform over the surface, area-weighted, stratified and seeded.  Meshes are as above.  No atomics on data, no host read,
 * no scratch block; two runs give bitwise-equal outputs; both calls capture into a graph.
 *
 * ms_mesh_face_areas: area[f] (T float64) = 0.5 |(b - a) x (c - a)| with (a, b, c) the positions of face f: differences,
 * products and the sum of squares (x x + y y) + z z are FLOAT64 operations on the float32 positions, without FMA
 * contraction.  status (1 int32, device; zeroed by the call) receives 0 or a sum of MS_MESH_BAD_INDEX (a face index
 * outside 0 .. V - 1; nothing is read through it) and MS_MESH_NOT_FINITE (a referenced vertex with a NaN or an infinity);
 * such a face gets area 0.  The caller makes the inclusive cumulative sum cdf (T float64) of the areas.
 *
 * ms_mesh_sample_points, for sample i of n (n < 2^31), with cdf[T - 1] > 0:
 *   t_i  = min((i + u0) (cdf[T - 1] / n), nextafter(cdf[T - 1], 0))        in float64: stratum i of n equal shares of area
 *   face = the first f with cdf[f] > t_i (a binary search): a face of area 0 is never drawn
 *   r = sqrt(u1), (wa, wb, wc) = (1 - r, r (1 - u2), r u2)                 in float32, sqrt correctly rounded
 *   out_points[i] = (wa A + wb B) + wc C per component                     in float32, without FMA contraction
 * out_face (n int32) and out_bary (n, 3) receive face and (wa, wb, wc); out_colours / out_normals (n, 3) the same
 * combination of the three rows of colours / normals (normals are NOT renormalised).  With normals == NULL, out_normals
 * is the unit face normal (b - a) x (c - a) / |.|, float64 rounded once.  Each of the four may be NULL.
 * RANDOM NUMBERS are counter-based, a function of (seed, i, j) alone, j = 0, 1, 2:
 *   mix(x):  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16      on uint32
 *   word(seed, i, j) = mix((uint32)i + mix((uint32)seed + 0x9e3779b9 (j + 1)))
 *   u_j = (word(seed, i, j) >> 8) 2^-24                                       24 bits in [0, 1): exact in float32
 * MS_ERR_BAD_ARG: sizes out of range, a null required pointer, n > 0 with V == 0 or T == 0, out_colours without colours. */
int ms_mesh_face_areas(const float* vertices, const int32_t* faces, int64_t num_vertices, int64_t num_faces,
                       double* area, int32_t* status, void* stream);
int ms_mesh_sample_points(const float* vertices, const int32_t* faces, const float* colours /* may be NULL */,
                          const float* normals /* may be NULL */, int64_t num_vertices, int64_t num_faces, const double* cdf,
                          int64_t n, int64_t seed, float* out_points, int32_t* out_face /* may be NULL */,
                          float* out_bary /* may be NULL */, float* out_colours /* may be NULL */,
                          float* out_normals /* may be NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355_SPLAT_H */
