"""Shared by tests/test_segment_cases_host.py (CPU) and tests/test_gpu_raster_segments.py: tile lists with CHOSEN run
lengths for the long-run segment kernels (ms_raster_fwd_split / ms_raster_bwd_moments_split; csrc/raster_common.h, "Long
tile runs"), the documented contract of their plan restated as properties of (tile, begin, end) items, a reader for the
plan a forward left in its scratch block, and the case table.

Lists.  ``confined_points`` draws ``cap`` gate-stable splats per tile whose footprints stay inside their tile
(tests/test_gpu_round6.py, ``confined_scene``, with the CPU mapper oracle.mapper.map_to_tiles), so every tile's list has
exactly ``cap`` entries; ``build`` then shortens tile t's range to (start, start + run_t).  The raster entry points and
oracle.raster take (overlap_to_point, tile_ranges) as given: ranges need not be contiguous, k_capacity is the length of
overlap_to_point.  Splats no shortened list names stay in the point arrays: their gradient rows must stay zero.

Contract (include/mi355_splat.h, "split_min_run / split_seg_len").  With min_run' and seg_len' the parameters after the
header's rules (0 = the defaults, values below 256 raised to 256, seg_len rounded up to a multiple of 256):

  cut        a tile has items iff its run has MORE than min_run' entries;
  covers     a tile's items are disjoint, contiguous and cover [start, end) exactly;
  length     all items of a tile but the last have one common length, a multiple of 256 and at least seg_len'; the last is
             no longer than that;
  count      a tile has at most 256 items.

No GPU is touched here and no device module is imported at module level."""
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from oracle import mapper as omap, raster as orast
from taichi_splatting_amd import RasterConfig

MAX_SEGMENTS = 256
DEFAULT_MIN_RUN = 16384
STABLE_MARGIN = 1e-4           # gate-stable: no (pixel, splat) pair within this (relative) of the blend gate
SATURATION_MARGIN = 1e-4       # rows with a pair this close to the backward's saturation limit are left out (saturating16)
LEFT_OUT_CAP = 0.01

EDGE_RUNS = (0, 1, 255, 511, 512, 513, 768, 1024, 1025, 1279, 1400, 1400)
# the same twelve runs, with cut and uncut tiles (at 512) in tile row 0 AND in tile rows 1..2 (4 tiles per row)
WINDOW_RUNS = (1400, 0, 513, 511, 1, 1025, 512, 768, 255, 1024, 1279, 1400)
EDGE_RUNS_32 = (0, 512, 513, 1024, 1025, 1400)


@dataclass(frozen=True)
class Case:
  name: str
  tile: int
  size: Tuple[int, int]
  runs: Tuple[int, ...]
  min_run: int                       # as PASSED to the entry points
  seg_len: int
  expect: Tuple[int, int]            # (min_run', seg_len') the kernels are expected to act on
  alpha_range: Tuple[float, float]
  inset: float
  seed: int
  alpha_threshold: Optional[float] = None      # None: RasterConfig's default
  saturating: bool = False
  visibility: bool = False           # the one configuration tests/test_gpu_raster_segments.py runs the case in
  heuristics: bool = False


def _case(name, tile, size, runs, split, expect=None, alpha_range=(0.01, 0.03), inset=4.0, seed=0, **kw):
  return Case(name, tile, size, tuple(runs), split[0], split[1], expect or split, alpha_range, inset, seed, **kw)


T8 = dict(alpha_range=(0.0045, 0.009), inset=2.5)
# one 8 x 8 tile, tens of thousands of entries: a gate of 8e-5 and opacities just above it keep the pixels short of saturation
DEEP8 = dict(alpha_range=(9e-5, 1.8e-4), inset=2.5, alpha_threshold=8e-5)
CASES = {c.name: c for c in (
  _case('edges16', 16, (64, 48), EDGE_RUNS, (512, 512), seed=1),
  _case('short_segments16', 16, (64, 48), EDGE_RUNS, (1024, 256), seed=1, visibility=True, heuristics=True),
  _case('one_segment16', 16, (64, 48), EDGE_RUNS, (256, 1024), seed=1, heuristics=True),
  _case('raised16', 16, (64, 48), EDGE_RUNS, (100, 1), expect=(256, 256), seed=1, visibility=True),
  _case('edges8', 8, (32, 24), EDGE_RUNS, (512, 512), seed=2, visibility=True, **T8),
  _case('edges32', 32, (96, 64), EDGE_RUNS_32, (512, 512), seed=3, heuristics=True),
  _case('deepest8', 8, (8, 8), (65536,), (256, 256), seed=4, heuristics=True, **DEEP8),
  _case('clamped8', 8, (8, 8), (65537,), (256, 256), seed=5, visibility=True, **DEEP8),
  # opacities at which the centre pixels of a tile reach the backward's saturation limit between entries 600 and 900
  _case('saturating16', 16, (64, 48), EDGE_RUNS, (512, 512), alpha_range=(0.2, 0.35), seed=6, saturating=True,
        visibility=True, heuristics=True),
  _case('window16', 16, (64, 48), WINDOW_RUNS, (512, 512), seed=7, heuristics=True),
)}
TABLE = tuple(n for n in CASES if n != 'window16')          # the issue's table; window16 = edges16's runs reordered


def config(case, **kw):
  """the case's RasterConfig (its own blend gate); ``kw`` overrides visibility / heuristics"""
  extra = {} if case.alpha_threshold is None else dict(alpha_threshold=case.alpha_threshold)
  kw.setdefault('compute_visibility', case.visibility)
  kw.setdefault('compute_point_heuristic', case.heuristics)
  return RasterConfig(tile_size=case.tile, pixel_stride=(1, 1) if case.tile == 8 else (2, 2), **extra, **kw)


def tiles_of(size, tile):
  return (size[0] + tile - 1) // tile, (size[1] + tile - 1) // tile


def confined_points(cap, size, tile, seed, alpha_range, alpha_threshold, inset, sigma=(0.5, 0.4), pool=1.5):
  """(points7 (n, 7), depth (n,), features (n, 3), share of the pool that was gate-stable), float32: ``cap`` gate-stable
  splats per tile, centres ``inset`` px inside their tile, sigma in [sigma0, sigma0 + sigma1) px.  A pool of ``pool * cap`` candidates per tile is drawn, the
  candidates with a pair within STABLE_MARGIN of the blend gate are dropped (a pair's margin does not depend on the
  other splats), the first ``cap`` of each tile kept.  Row layout: mean, axis, sigma, opacity."""
  tw, th = tiles_of(size, tile)
  tiles = tw * th
  n = int(cap * pool) * tiles
  gen = torch.Generator().manual_seed(seed)
  rand = lambda *shape: torch.rand(*shape, generator=gen)
  owner = torch.arange(n) % tiles
  span = tile - 2 * inset
  mean = torch.stack([(owner % tw) * tile + inset + span * rand(n), (owner // tw) * tile + inset + span * rand(n)], 1)
  axis = torch.randn(n, 2, generator=gen)
  axis = axis / axis.norm(dim=1, keepdim=True)
  sig = sigma[0] + sigma[1] * rand(n, 2)
  alpha = alpha_range[0] + (alpha_range[1] - alpha_range[0]) * rand(n, 1)
  p = torch.cat([mean, axis, sig, alpha], 1).float()
  depth, f = rand(n).float(), rand(n, 3).float()
  cfg = orast.Cfg(tile_size=tile, alpha_threshold=alpha_threshold)
  o2p, ranges, _ = omap.map_to_tiles(p.numpy(), depth.numpy(), size, tile, alpha_threshold)
  margin = orast.gate_margin(p.double(), torch.from_numpy(ranges).reshape(-1, 2), torch.from_numpy(o2p), size, cfg)
  stable = margin > STABLE_MARGIN
  keep = torch.zeros(n, dtype=torch.bool)
  for t in range(tiles):
    idx = torch.nonzero(stable & (owner == t)).squeeze(1)
    assert idx.numel() >= cap, (t, idx.numel(), cap)
    keep[idx[:cap]] = True
  return p[keep].contiguous(), depth[keep].contiguous(), f[keep].contiguous(), float(stable.float().mean())


@dataclass(frozen=True)
class Built:
  case: Case
  p: torch.Tensor            # (n, 7) float32
  depth: torch.Tensor        # (n,)
  f: torch.Tensor            # (n, 3)
  o2p: torch.Tensor          # (K,) int32: the FULL lists (cap entries per tile)
  ranges: torch.Tensor       # (tiles, 2) int32: shortened to the case's runs
  stable_share: float        # share of the drawn pool that was gate-stable

  @property
  def listed(self):
    """(n,) bool: splats some shortened list names"""
    out = torch.zeros(self.p.shape[0], dtype=torch.bool)
    for s, e in self.ranges.tolist():
      out[self.o2p[s:e].long()] = True
    return out


@functools.lru_cache(maxsize=None)
def build(name):
  case = CASES[name]
  cfg = config(case)
  tw, th = tiles_of(case.size, case.tile)
  assert len(case.runs) == tw * th, (name, len(case.runs), tw * th)
  cap = max(case.runs)
  p, depth, f, share = confined_points(cap, case.size, case.tile, case.seed, case.alpha_range, cfg.alpha_threshold, case.inset,
                                       pool=1.1 if cap > 4096 else 1.5)
  o2p, ranges, _ = omap.map_to_tiles(p.numpy(), depth.numpy(), case.size, case.tile, cfg.alpha_threshold)
  ranges = torch.from_numpy(ranges).reshape(-1, 2).clone()
  full = ranges[:, 1] - ranges[:, 0]
  assert int(full.min()) == cap == int(full.max()), (name, int(full.min()), int(full.max()), cap)     # confined: nothing leaks
  ranges[:, 1] = ranges[:, 0] + torch.tensor(case.runs, dtype=torch.int32)
  return Built(case, p, depth, f, torch.from_numpy(o2p).contiguous(), ranges.contiguous(), share)


FRAME_TILE, FRAME_SIZE = 16, (64, 48)
# per tile of the frame-executor scene: 1400 splats on half the tiles, 300 on a quarter, none on the rest
FRAME_COUNTS = tuple((1400, 300, 1400, 0)[t % 4] for t in range(12))


@functools.lru_cache(maxsize=None)
def frame_scene(seed=8):
  """(points7, depth, features): a confined scene with FRAME_COUNTS[t] splats centred in tile t, for a frame that maps
  them itself (the points are thinned, not the lists)"""
  p, depth, f, _ = confined_points(max(FRAME_COUNTS), FRAME_SIZE, FRAME_TILE, seed, (0.01, 0.03), RasterConfig().alpha_threshold, 4.0)
  tw, _ = tiles_of(FRAME_SIZE, FRAME_TILE)
  owner = (p[:, 0] / FRAME_TILE).floor().long() + (p[:, 1] / FRAME_TILE).floor().long() * tw
  keep = torch.zeros(p.shape[0], dtype=torch.bool)
  for t, count in enumerate(FRAME_COUNTS):
    keep[torch.nonzero(owner == t).squeeze(1)[:count]] = True
  return p[keep].contiguous(), depth[keep].contiguous(), f[keep].contiguous()


def grad_image(size, seed=1):
  """dL/dimage (H, W, 3) float32, positive, as the segment tests of tests/test_gpu_round6.py use"""
  return (torch.rand(size[1], size[0], 3, generator=torch.Generator().manual_seed(seed)) + 0.5).contiguous()


@functools.lru_cache(maxsize=None)
def oracle(name, tile_rows=None):
  """the float64 oracle of a case on its own lists: dict of image, alpha, visibility, grad_points, grad_features,
  heuristics (none depends on the visibility / heuristics switches: they only select what a kernel computes).  Computed
  once per (case, window) and shared: do not write into it."""
  b = build(name)
  cfg = config(b.case)
  p64, f64, G = b.p.double(), b.f.double(), grad_image(b.case.size).double()
  image, alpha, vis = orast.forward(p64, f64, b.ranges, b.o2p, b.case.size, cfg, tile_rows=tile_rows)
  gp, gf, heur = orast.backward(p64, f64, b.ranges, b.o2p, image, G, b.case.size, cfg, tile_rows=tile_rows)
  return dict(image=image, alpha=alpha, visibility=vis, grad_points=gp, grad_features=gf, heuristics=heur)


def compared_rows(name):
  """(n,) bool: the gradient rows a saturating case is compared on — those without a (pixel, splat) pair within
  SATURATION_MARGIN of the backward's saturation limit (tests/test_gpu_raster_wide.py); None for the other cases"""
  b = build(name)
  if not b.case.saturating:
    return None
  margin, _ = orast.saturation_margin(b.p.double(), b.ranges, b.o2p, b.case.size, config(b.case))
  return margin >= SATURATION_MARGIN


def first_saturated_entry(name):
  """(H, W) int: position in its tile's list of the first entry a pixel's backward drops for saturation, -1 if none"""
  from .threshold_cases import first_saturated_entry as first
  b = build(name)
  return first(b.p, b.ranges, b.o2p, b.case.size, config(b.case))


# ---- the plan ---------------------------------------------------------------------------------------------------------
def effective_params(min_run, seg_len, tile):
  """(min_run', seg_len') after the header's rules"""
  m = DEFAULT_MIN_RUN if min_run == 0 else max(min_run, 256)
  s = (4096 if tile == 32 else 1024) if seg_len == 0 else max((seg_len + 255) // 256 * 256, 256)
  return m, s


def expected_segments(run, min_run, seg_len):
  """The plan split_plan_kernel makes of one run, EFFECTIVE parameters: [] if the run is not cut, else the segment
  lengths.  The contract leaves the kernel room (any common length >= seg_len' will do); the kernel takes
  ceil(run / seg_len') segments, 256 at most, of equal length rounded up to a multiple of 256 and raised to seg_len'.
  The case table reaches its edges — a last segment of one entry, a long tile of one item, 256 items — through this
  choice, so the host test states it and the device test compares the device's plan with it."""
  if run <= min_run:
    return []
  ceil_div = lambda a, b: (a + b - 1) // b
  nseg = min(ceil_div(run, seg_len), MAX_SEGMENTS)
  length = max(ceil_div(ceil_div(run, nseg), 256) * 256, seg_len)
  nseg = ceil_div(run, length)
  return [length] * (nseg - 1) + [run - length * (nseg - 1)]


PROPERTIES = ('cut', 'covers', 'length', 'count')


def plan_violations(items, ranges, min_run, seg_len, tile_rows=None, tiles_wide=None):
  """The contract of the module docstring on ``items`` = iterable of (tile, begin, end) for lists ``ranges`` (tiles, 2) and
  EFFECTIVE parameters: a list of (property, tile, detail), empty if the plan keeps the contract.  ``tile_rows``
  = (begin, end) with ``tiles_wide``: only tiles of those rows may (and, if long, must) have items."""
  by_tile = {}
  for tile, b, e in items:
    by_tile.setdefault(int(tile), []).append((int(b), int(e)))
  ranges = [(int(s), int(e)) for s, e in np.asarray(ranges).reshape(-1, 2)]
  bad = []
  for tile in by_tile:
    if not 0 <= tile < len(ranges):
      bad.append(('cut', tile, 'no such tile'))
  for tile, (start, end) in enumerate(ranges):
    segs = sorted(by_tile.get(tile, []))
    inside = tile_rows is None or tile_rows[0] * tiles_wide <= tile < tile_rows[1] * tiles_wide
    long = end - start > min_run and inside
    if long != bool(segs):
      bad.append(('cut', tile, f'run {end - start}, min_run {min_run}, {len(segs)} items'))
    if not segs:
      continue
    edges_ok = segs[0][0] == start and segs[-1][1] == end and all(b < e for b, e in segs) and \
      all(segs[i][1] == segs[i + 1][0] for i in range(len(segs) - 1))
    if not edges_ok:
      bad.append(('covers', tile, f'[{start}, {end}) by {segs[:4]}{"..." if len(segs) > 4 else ""}'))
    lengths = [e - b for b, e in segs]
    common = lengths[:-1]
    if common and (len(set(common)) != 1 or common[0] % 256 != 0 or common[0] < seg_len or lengths[-1] > common[0]):
      bad.append(('length', tile, f'lengths {sorted(set(common))} then {lengths[-1]}, seg_len {seg_len}'))
    if len(segs) > MAX_SEGMENTS:
      bad.append(('count', tile, f'{len(segs)} items'))
  return bad


def carve(k_capacity, tile, min_run, seg_len):
  """split_scratch_carve restated for EFFECTIVE parameters: byte offsets of (long_tiles, items, state), the two
  capacities and the block's size.  256 bytes of counts, then long_cap and item_cap 16-byte records, each array padded
  to 256 bytes, then item_cap x tile^2 16-byte states."""
  long_cap = k_capacity // min_run + 1
  item_cap = k_capacity // seg_len + long_cap + 1
  pad = lambda n: (n + 255) // 256 * 256
  long_off = 256
  item_off = long_off + pad(long_cap * 16)
  state_off = item_off + pad(item_cap * 16)
  return dict(long_tiles=long_off, items=item_off, state=state_off, long_cap=long_cap, item_cap=item_cap,
              bytes=state_off + item_cap * tile * tile * 16)


def read_plan(scratch, k_capacity, tile, min_run, seg_len):
  """``scratch``: a CPU copy (uint8 tensor or array) of the block a forward has written; EFFECTIVE parameters.  Returns
  (counts (4,), long_tiles (counts[1], 4) = (tile, first item, segments, 0), items (counts[0], 4) = (tile, begin, end,
  the tile's first item)) as int64 arrays.  Counts beyond the capacities (a plan that did not fit) are clipped."""
  raw = np.ascontiguousarray(scratch.numpy() if isinstance(scratch, torch.Tensor) else scratch, dtype=np.uint8)
  c = carve(k_capacity, tile, min_run, seg_len)
  words = lambda off, n: raw[off:off + 16 * n].view(np.int32).reshape(n, 4).astype(np.int64)
  counts = raw[:16].view(np.int32).astype(np.int64)
  return counts, words(c['long_tiles'], min(int(counts[1]), c['long_cap'])), words(c['items'], min(int(counts[0]), c['item_cap']))


def check_plan(counts, long_tiles, items, ranges, min_run, seg_len, tile_rows=None, tiles_wide=None):
  """§b of the device test, for any plan: the contract, the three counts, and that the long-tile records and the items
  name each other.  Returns {tile: [segment lengths]}."""
  bad = plan_violations(items[:, :3], ranges, min_run, seg_len, tile_rows, tiles_wide)
  assert not bad, bad
  runs = np.asarray(ranges).reshape(-1, 2)
  runs = runs[:, 1] - runs[:, 0]
  if tile_rows is not None:
    inside = np.arange(runs.shape[0]) // tiles_wide
    runs = runs[(inside >= tile_rows[0]) & (inside < tile_rows[1])]
  assert int(counts[2]) == 0, counts
  assert int(counts[1]) == int((runs > min_run).sum()) == long_tiles.shape[0], (counts, int((runs > min_run).sum()))
  assert int(counts[0]) == items.shape[0] == int(long_tiles[:, 2].sum()), (counts, items.shape)
  segments = {}
  for tile, first, nseg, _ in long_tiles.tolist():
    mine = items[first:first + nseg]                         # a tile's items are consecutive, front to back
    assert bool((mine[:, 0] == tile).all()) and bool((mine[:, 3] == first).all()), (tile, first, nseg)
    assert bool((np.diff(mine[:, 1]) > 0).all()), (tile, 'items out of order')
    assert tile not in segments, (tile, 'two long-tile records')
    segments[tile] = (mine[:, 2] - mine[:, 1]).tolist()
  assert sum(len(v) for v in segments.values()) == items.shape[0]
  return segments
