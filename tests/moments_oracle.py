"""Float64 oracle of the raster backward's MOMENT ROWS (include/mi355_splat.h, the block above MS_MOMENT_ROW), of the pass
that turns them into gradients (raster_moments_finalize_kernel, csrc/raster_bwd_scan.hip) and of the kernels that choose
the fixed-point units of the deterministic mode (ms_fixed_point_exponents / ms_fixed_point_exponents_ranged).

Plain torch on the oracle's tile lists: the per-(pixel, splat) quantities are those of ``oracle.raster.backward`` — same
``_tile_pixels`` and ``pdf``, same blend gate, clamp and saturation rule — summed per splat into the twelve columns the
kernel commits instead of into gradients.

How often a row is committed (read from ``commit_pass`` and the batch loop of raster_bwd_scan_kernel): a wave owns one
8 x 8 pixel patch; a tile's list is cut into batches and a batch into passes; a staged splat is in exactly one batch and,
by the cull loop's ``r`` cursor, in exactly one pass of it, and ``commit_pass`` issues one atomic per (row of the pass,
column) whose sum is not zero.  A list holds a splat once, so a (patch, splat, column) is committed AT MOST ONCE.  That
holds for tile 8 (one wave per tile), tile 16 (four waves), tile 32 (sixteen waves, or four quarter workgroups with four
waves each: every patch still belongs to one wave) and for the segment kernels (a long run is cut into segments, each
entry of the run is in one segment; the per-tile kernel skips the tiles the segments take).  ``P[i]`` — the patches with
a pixel where the pair's raw alpha exceeds ``alpha_threshold (1 - 1e-3)``: a float32 gate cannot pass elsewhere —
therefore bounds the number of commits of every column of row i."""
import math

import torch

from oracle import raster as orast

BASIS_SCALE = math.sqrt(math.log2(math.e) / 2)       # (X', Y') = BASIS_SCALE * the pixel in the splat's normalised frame
FIXED_POINT_BITS = 36
VISIBILITY_EXPONENT = 32                             # column 11: units of 2^-32


def moment_rows(points, feats, ranges, o2p, image, grad_image, image_size, cfg):
  """M (V, 12), A (V, 12), P (V,) int64, dropped (V,): the sums, the sums of the absolute values of their per-pixel
  terms, the patch counts (module docstring) and the blend weight of the pairs behind a pixel's saturation point (what
  ``oracle.raster.forward``'s visibility holds beyond column 11).  float64 tensors on the CPU; ``image`` is the forward's."""
  w, h = image_size
  ts = cfg.tile_size
  tiles_wide, tiles_high = orast._tiles(image_size, ts)
  dtype = torch.float64
  points, feats, image, grad_image = (t.detach().cpu().to(dtype) for t in (points, feats, image, grad_image))
  ranges, o2p = ranges.cpu().reshape(-1, 2), o2p.cpu()
  V = points.shape[0]
  M, A = torch.zeros((V, 12), dtype=dtype), torch.zeros((V, 12), dtype=dtype)
  P = torch.zeros((V,), dtype=torch.int64)
  dropped = torch.zeros((V,), dtype=dtype)
  patches_wide = (w + 7) // 8
  for tile_id in range(tiles_wide * tiles_high):
    start, end = int(ranges[tile_id, 0]), int(ranges[tile_id, 1])
    if end <= start:
      continue
    px, py, inb, pix = orast._tile_pixels(tile_id, tiles_wide, ts, w, h, dtype)
    pix, px, py = pix[inb], px[inb], py[inb]
    n_pix = pix.shape[0]
    if n_pix == 0:
      continue
    ids = o2p[start:end].long()
    g, f = points[ids], feats[ids]
    C_final, G = image[py, px], grad_image[py, px]
    p = orast.pdf(pix, g, False)
    pa = g[None, :, 6]
    a_raw = pa * p
    gate = a_raw > cfg.alpha_threshold
    a_all = torch.where(gate, torch.clamp_max(a_raw, cfg.clamp_max_alpha), torch.zeros_like(a_raw))
    T_incl = torch.cumprod(1 - a_all, dim=1)
    T_excl = torch.cat([torch.ones((n_pix, 1), dtype=dtype), T_incl[:, :-1]], dim=1)
    active = gate & ((1 - T_excl) < cfg.saturate_threshold)
    a = torch.where(active, a_all, torch.zeros_like(a_all))
    weight = a * T_excl
    prefix = torch.cumsum(weight[:, :, None] * f[None], dim=1)
    R = C_final[:, None, :] - prefix
    diff = f[None] * T_excl[:, :, None] - R / (1 - a)[:, :, None]
    ag = torch.where(active, (diff * G[:, None, :]).sum(-1), torch.zeros_like(a))        # dL/dalpha
    q = a_raw * ag                                       # straight-through clamp: alpha_pt g dL/dalpha

    mean, axis, sigma = g[:, 0:2], g[:, 2:4], g[:, 4:6]
    d = pix[:, None, :] - mean[None]
    X = BASIS_SCALE * (d * axis[None]).sum(-1) / sigma[None, :, 0]
    Y = BASIS_SCALE * (d * orast.perp(axis)[None]).sum(-1) / sigma[None, :, 1]
    bA, bB = BASIS_SCALE * axis[:, 0] / sigma[:, 0], BASIS_SCALE * axis[:, 1] / sigma[:, 0]
    bC, bD = -BASIS_SCALE * axis[:, 1] / sigma[:, 1], BASIS_SCALE * axis[:, 0] / sigma[:, 1]
    l1 = (X * bA[None] + Y * bC[None]).abs() + (X * bB[None] + Y * bD[None]).abs()
    terms = torch.stack([q, q * X, q * Y, q * X * X, q * X * Y, q * Y * Y,
                         weight * G[:, None, 0], weight * G[:, None, 1], weight * G[:, None, 2],
                         ag * ag, q.abs() * l1, weight], dim=-1)                         # (pixels, splats, 12)
    M.index_add_(0, ids, terms.sum(0))
    A.index_add_(0, ids, terms.abs().sum(0))
    dropped.index_add_(0, ids, (torch.where(active, torch.zeros_like(a_all), a_all) * T_excl).sum(0))

    near = a_raw > cfg.alpha_threshold * (1 - 1e-3)
    patch = ((py // 8) * patches_wide + px // 8).long()
    for k in torch.unique(patch):
      P.index_add_(0, ids, near[patch == k].any(dim=0).long())
  return M, A, P, dropped


def finalize(points, M):
  """raster_moments_finalize_kernel in float64: (grad_points (V, 7), grad_features (V, 3), heuristics (V, 2),
  column 11).  Rows that can never blend (alpha or a sigma not positive) get zero gradients, as the kernel's do."""
  points, M = points.detach().cpu().double(), M.double()
  ax, ay, sx, sy, alpha = (points[:, k] for k in (2, 3, 4, 5, 6))
  dead = ~(alpha > 0) | ~(sx > 0) | ~(sy > 0)
  one = torch.ones_like(sx)
  isx, isy = one / torch.where(dead, one, sx), one / torch.where(dead, one, sy)
  bA, bB, bC, bD = ax * isx, ay * isx, -ay * isy, ax * isy
  IS = 1.0 / BASIS_SCALE
  S, Sx, Sy = M[:, 0], M[:, 1] * IS, M[:, 2] * IS
  Sxx, Sxy, Syy = M[:, 3] * IS * IS, M[:, 4] * IS * IS, M[:, 5] * IS * IS
  det = bA * bD - bB * bC
  idet = torch.where(det != 0, one / torch.where(det != 0, det, one), torch.zeros_like(det))
  gp = torch.stack([Sx * bA + Sy * bC, Sx * bB + Sy * bD,
                    -(isx * (bD * Sxx - bB * Sxy) + isy * (bA * Syy - bC * Sxy)) * idet,
                    (isy * (bD * Sxy - bB * Syy) + isx * (bC * Sxx - bA * Sxy)) * idet,
                    isx * Sxx, isy * Syy, S / torch.where(dead, one, alpha)], dim=1)
  gp = torch.where(dead[:, None], torch.zeros_like(gp), gp)
  heur = torch.stack([alpha * alpha * M[:, 9], M[:, 10] * IS * IS], dim=1)
  return gp, M[:, 6:9].clone(), heur, M[:, 11].clone()


def _clamp100(e):
  return max(-100, min(100, e))


def _exponent(x):
  """frexp's exponent of a float32 value that is positive and finite, else None"""
  return math.frexp(x)[1] if (x > 0.0 and x < math.inf) else None


def _f32(x):
  return float(torch.tensor(x, dtype=torch.float32))


def exponents(amax):
  """fixed_point_exponents_kernel: (e_main, e_h0) from max |dL/dimage| alone"""
  e = _exponent(_f32(amax)) or 0
  return _clamp100(FIXED_POINT_BITS - e), _clamp100(FIXED_POINT_BITS - 2 * e)


def exponents_ranged(amax, fmax, smin, pixels, alpha_threshold):
  """ms_fixed_point_exponents_ranged (host part and kernel), in the same whole binary exponents"""
  amax, fmax, smin, thr = _f32(amax), _f32(fmax), _f32(smin), _f32(alpha_threshold)
  log2_pixels = 0
  while log2_pixels < 62 and (1 << log2_pixels) < pixels:
    log2_pixels += 1
  L = -math.log2(thr) if thr > 0.0 else 160.0
  if not L >= 1.0:
    L = 1.0
  L = min(L, 160.0)
  log2_L = 0
  while float(1 << log2_L) < L:
    log2_L += 1
  e = _exponent(amax) or 0
  f_known = fmax >= 0.0 and fmax < math.inf
  e_f = 128 if not f_known else (_exponent(fmax) or 0)
  e_s = _exponent(smin)
  e_s = 1 if e_s is None else e_s
  geom = max(log2_L, 2 + (log2_L + 1) // 2 - e_s)
  zero = f_known and fmax == 0.0
  h_main = 0 if zero else max(0, 3 + e_f + geom)
  h_h0 = 0 if zero else max(0, 6 + 2 * e_f)
  free = 61 - FIXED_POINT_BITS
  return (_clamp100(FIXED_POINT_BITS - e - max(0, h_main + log2_pixels - free)),
          _clamp100(FIXED_POINT_BITS - 2 * e - max(0, h_h0 + log2_pixels - free)))


def launch_stats(points, feats, grad_image):
  """(max |dL/dimage|, max |feature|, smallest positive sigma) as ``_lib.fixed_point_exponents_ranged`` reduces them"""
  feats, sigma = feats.detach().float(), points.detach().float()[:, 4:6]
  fmax = torch.where(torch.isfinite(feats), feats.abs(), torch.zeros_like(feats)).amax()
  smin = torch.where(sigma > 0, sigma, torch.full_like(sigma, math.inf)).amin()
  return float(grad_image.detach().float().abs().amax()), float(fmax), float(smin)


def column_units(e_main, e_h0):
  """(12,) float64: the unit 2^-e of every column"""
  u = torch.full((12,), 2.0 ** -e_main, dtype=torch.float64)
  u[9] = 2.0 ** -e_h0
  u[11] = 2.0 ** -VISIBILITY_EXPONENT
  return u


# ---- the headroom scene: a background splat over the whole image, with colours of magnitude M ---------------------------
HEADROOM_SIZE = (256, 256)
# (M, alpha of the background splat, G, the column the case is aimed at or None for the control)
HEADROOM_CASES = {
  'control': (1.0, 0.5, 1.0, None),
  'linear': (4000.0, 0.5, 1.0, 0),
  'squared': (100.0, 0.9, 1.0, 9),
  'linear_negative': (4000.0, 0.5, -1.0, 0),
}


def headroom_scene(colour, alpha):
  """(points7 (2, 7), features (2, 3), depth (2,)) float32: a sigma-400 splat of colour (M, M, M) behind a small one"""
  p = torch.tensor([[128, 128, 1, 0, 400, 400, alpha], [40, 60, 1, 0, 3, 2, 0.6]], dtype=torch.float32)
  f = torch.tensor([[colour, colour, colour], [0.3, 0.5, 0.7]], dtype=torch.float32)
  return p, f, torch.tensor([2.0, 1.0], dtype=torch.float32)


def oracle_lists(p, depth, size, cfg):
  from oracle import mapper as omap
  o2p, ranges, _ = omap.map_to_tiles(p.numpy(), depth.numpy(), size, cfg.tile_size, cfg.alpha_threshold)
  return torch.from_numpy(o2p), torch.from_numpy(ranges).reshape(-1, 2)
