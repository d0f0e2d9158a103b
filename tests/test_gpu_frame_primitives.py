"""-m gpu: the variants of the integer primitives that exist only inside the frame executor — the adaptive depth pre-sort
(``radix_sort_depth_adaptive``), the device-count sorts (``sort_pairs_u32_dev_launch`` / ``sort_ids_payload_dev_launch``) and
the range kernels ``find_ranges4_kernel`` / ``find_ranges_ids_kernel`` of csrc/scan_sort.hip — driven through the C-ABI
(``ms_frame_layout_query``, ``ms_frame_project_count``, ``ms_frame_map_raster``) with inputs that choose the route of the
pre-sort and the overlap total K to the element.

Projected input (the test supplies packed 2D gaussians, depths and colours) with ``near_plane = 0``: the sort key is the
float bit pattern of the depth.  Splats that overlap exactly one tile: K = n.  Cases and references:
tests/primitive_cases.py, held to what they claim by tests/test_primitive_cases_host.py.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import mapper as omap
from taichi_splatting_amd import RasterConfig, _lib
from tests import primitive_cases as pc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MAPPERS = {'direct': _lib.MAPPER_DIRECT, 'presort': _lib.MAPPER_PRESORT}
POISON = 0xAB          # the caller's blocks are not zeroed by the product either (torch.empty)


class Frame:
  """One frame through the C-ABI: ``project_count()``, then ``map_raster()``; views of the arrays the primitives write."""

  def __init__(self, n, image_size, tile_size, mapper, k_capacity, depth16=False, projected=True, depth_range=(0.0, 0.0),
               points7=None, depth=None, colours=None, gaussians=None):
    self.lib = _lib.load()
    self.n, self.k_capacity = n, k_capacity
    w, h = image_size
    cfg = RasterConfig(tile_size=tile_size, pixel_stride=(1, 1) if tile_size == 8 else (2, 2))
    self.tiles_wide, self.tiles_high = (w + tile_size - 1) // tile_size, (h + tile_size - 1) // tile_size
    self.num_tiles = self.tiles_wide * self.tiles_high
    self.desc = _lib.FrameDescC(n=n, k_capacity=k_capacity, image_w=w, image_h=h, dtype=_lib.MS_F32, f=3, sh_degree=-1,
                                depth16=int(depth16), tile_row_begin=0, tile_row_end=self.tiles_high,
                                projected_input=int(projected), mapper=mapper, split_long_runs=0, split_seg_len=0,
                                sh_active_bands=0, near_plane=float(depth_range[0]), far_plane=float(depth_range[1]),
                                blur_cov=cfg.blur_cov, clamp_margin=cfg.clamp_margin, raster=_lib.raster_config_c(cfg))
    self.lay = _lib.FrameLayoutC()
    _lib.check(self.lib.ms_frame_layout_query(ctypes.byref(self.desc), ctypes.byref(self.lay)), "layout")
    block = lambda nbytes: torch.full((max(int(nbytes), 1),), POISON, dtype=torch.uint8, device=DEV)
    self.keep_n, self.scratch_n = block(self.lay.keep_n_bytes), block(self.lay.scratch_n_bytes)
    self.keep_k, self.scratch_k = block(self.lay.keep_k_bytes), block(self.lay.scratch_k_bytes)
    dev = lambda a: None if a is None else torch.as_tensor(a, dtype=torch.float32).contiguous().to(DEV)
    if projected:
      self.held = [dev(points7), dev(depth), dev(colours if colours is not None else np.full((n, 3), 0.5, dtype=np.float32))]
      self.inputs = _lib.FrameInputsC(points7=self.held[0].data_ptr(), depth=self.held[1].data_ptr(), colours=self.held[2].data_ptr())
    else:
      self.held = [dev(a) for a in gaussians]       # position, log_scaling, rotation, alpha_logit, feature, T_camera_world, projection
      names = ('position', 'log_scaling', 'rotation', 'alpha_logit', 'feature', 'T_camera_world', 'projection')
      self.inputs = _lib.FrameInputsC(**{name: t.data_ptr() for name, t in zip(names, self.held)})
    self.stream = _lib.current_stream(torch.device(DEV))
    self.image = torch.empty((h, w, 3), dtype=torch.float32, device=DEV)
    self.alpha = torch.empty((h, w), dtype=torch.float32, device=DEV)

  def project_count(self):
    _lib.check(self.lib.ms_frame_project_count(ctypes.byref(self.desc), ctypes.byref(self.inputs), self.keep_n.data_ptr(),
                                               self.scratch_n.data_ptr(), None, None, self.stream), "project_count")
    torch.cuda.synchronize()
    return self

  def map_raster(self):
    _lib.check(self.lib.ms_frame_map_raster(ctypes.byref(self.desc), ctypes.byref(self.inputs), self.keep_n.data_ptr(),
                                            self.scratch_n.data_ptr(), self.keep_k.data_ptr(), self.scratch_k.data_ptr(),
                                            self.image.data_ptr(), self.alpha.data_ptr(), None, self.stream), "map_raster")
    torch.cuda.synchronize()
    return self

  @staticmethod
  def _view(block, offset, dtype, shape):
    count = int(np.prod(shape))
    return block[offset:offset + count * torch.empty((), dtype=dtype).element_size()].view(dtype).view(*shape).cpu().numpy()

  @property
  def sorted_keys(self):        # scratch_n: (n,) uint32 keys of the depth pre-sort, ascending
    return self._view(self.scratch_n, self.lay.sorted_keys, torch.int32, (self.n,)).view(np.uint32)

  @property
  def order(self):              # scratch_n: (n,) the pre-sort's permutation
    return self._view(self.scratch_n, self.lay.order, torch.int32, (self.n,))

  @property
  def counters(self):           # keep_n: [0] K, [1] live K (0 on overflow), [2] overflow flag
    return self._view(self.keep_n, self.lay.counters, torch.int32, (8,))

  @property
  def tile_ranges(self):
    return self._view(self.keep_n, self.lay.tile_ranges, torch.int32, (self.num_tiles, 2))

  @property
  def depth(self):              # keep_n: the frame's own depths (not with projected input)
    return self._view(self.keep_n, self.lay.depth, torch.float32, (self.n,))

  @property
  def points7(self):
    return self._view(self.keep_n, self.lay.points7, torch.float32, (self.n, 7))

  def overlap_to_point(self, k):
    return self._view(self.keep_k, self.lay.overlap_to_point, torch.int32, (k,))


# ---- adaptive depth pre-sort: every route --------------------------------------------------------------------------------

GRID_A = pc.GRIDS['13x7_t16']


def _presort(depth, depth16=False):
  n = depth.shape[0]
  tiles = pc.tile_assignment('round_robin', n, GRID_A[0] * GRID_A[1])
  return Frame(n, pc.image_size(GRID_A), GRID_A[2], _lib.MAPPER_PRESORT, 0, depth16=depth16,
               points7=pc.one_tile_splats(tiles, GRID_A), depth=depth).project_count()


@pytest.mark.parametrize('n', pc.VARY_SIZES)
@pytest.mark.parametrize('mask', range(16), ids=lambda m: f"{m:04b}")
def test_adaptive_presort_every_vary_mask(mask, n):
  """keys that differ in exactly the bytes of ``mask``: passes 1..3 run or are skipped accordingly, the active ones chain
  through the two alternate buffers and the last active one writes the caller's arrays"""
  keys = pc.vary_keys(mask, n)
  f = _presort(keys.view(np.float32))
  want = np.argsort(keys, kind='stable')
  assert np.array_equal(f.order, want.astype(np.int32))
  assert np.array_equal(f.sorted_keys, keys[want])
  assert int(f.counters[0]) == n                      # one tile per splat: the overlap scan behind the pre-sort gives K = n


@pytest.mark.parametrize('n', pc.VARY_SIZES)
@pytest.mark.parametrize('kind', list(pc.DEPTH16_KINDS))
def test_adaptive_presort_depth16_routes(kind, n):
  depth, _ = pc.depth16_depths(kind, n)
  keys = omap.depth_key_bits(depth, True).astype(np.uint32)
  f = _presort(depth, depth16=True)
  want = np.argsort(keys, kind='stable')
  assert np.array_equal(f.order, want.astype(np.int32))
  assert np.array_equal(f.sorted_keys, keys[want])


def _three_depth_scene(n, size):
  """gaussians at camera depths 2, 3.5 and 5 in front of an identity camera, every fifth mirrored behind it"""
  rng = np.random.default_rng(5)
  w, h = size
  fx = fy = 0.9 * w
  z = np.asarray([2.0, 3.5, 5.0])[rng.integers(0, 3, size=n)]
  px, py = rng.uniform(2, w - 2, size=n), rng.uniform(2, h - 2, size=n)
  position = np.stack([(px - w / 2) * z / fx, (py - h / 2) * z / fy, z], axis=1)
  position[::5] *= -1.0
  log_scaling = np.log(rng.uniform(0.5, 3.0, size=(n, 3)) * (z / fx)[:, None])
  rotation = rng.normal(size=(n, 4))
  rotation /= np.linalg.norm(rotation, axis=1, keepdims=True)
  alpha_logit = rng.uniform(-1.0, 2.0, size=(n, 1))
  feature = rng.uniform(0, 1, size=(n, 3))
  T = np.eye(4)
  projection = np.asarray([fx, fy, w / 2, h / 2])
  return [a.astype(np.float32) for a in (position, log_scaling, rotation, alpha_logit, feature, T, projection)]


@pytest.mark.parametrize('mapper', list(MAPPERS))
def test_culled_rows_sort_last_or_not_at_all_and_lists_match_oracle(mapper):
  """the frame's own projection: culled gaussians (depth 0) carry the key 0xffffffff, stay out of the vary mask, appear
  once each in the pre-sort's order, and the tile lists are the oracle's on the visible rows"""
  n, size, ts = 3 * pc.RS_TILE + 5, (208, 112), 16
  near, far = 0.1, 100.0
  f = Frame(n, size, ts, MAPPERS[mapper], 16 * n, projected=False, depth_range=(near, far),
            gaussians=_three_depth_scene(n, size)).project_count()
  depth = f.depth
  visible = depth > 0
  vis_idx = np.flatnonzero(visible)
  assert n // 5 <= (~visible).sum() < n // 2 and np.unique(depth[visible]).shape[0] == 3

  depth_dev = torch.from_numpy(depth).to(DEV)
  keys_dev = torch.empty(n, dtype=torch.int32, device=DEV)
  vals_dev = torch.empty(n, dtype=torch.int32, device=DEV)
  _lib.check(f.lib.ms_depth_sort_keys(depth_dev.data_ptr(), n, 0, near, far, keys_dev.data_ptr(), vals_dev.data_ptr(),
                                      _lib.MS_F32, f.stream), "keys")
  keys = keys_dev.cpu().numpy().view(np.uint32)

  if mapper == 'presort':
    order, sorted_keys = f.order, f.sorted_keys
    assert np.array_equal(np.sort(order), np.arange(n)), "order is a permutation: every row once"
    want_vis = vis_idx[np.argsort(keys[vis_idx], kind='stable')]
    assert np.array_equal(order[visible[order]], want_vis.astype(np.int32))
    assert np.array_equal(sorted_keys[visible[order]], keys[want_vis])
    assert (sorted_keys[~visible[order]] == 0xffffffff).all()

  K = int(f.counters[0])
  assert 0 < K <= f.k_capacity
  f.map_raster()
  assert f.counters[:3].tolist() == [K, K, 0]
  o2p, ranges, counts = omap.map_to_tiles(f.points7[vis_idx], keys[vis_idx].view(np.float32), size, ts, 1. / 255.)
  assert int(counts.sum()) == K
  assert np.array_equal(f.tile_ranges, ranges.reshape(-1, 2))
  assert np.array_equal(f.overlap_to_point(K), vis_idx[o2p].astype(np.int32))


# ---- chosen K ------------------------------------------------------------------------------------------------------------

def _run_chosen(grid, tiles, mapper, k_capacity, seed=0):
  """(frame after both calls, expected overlap_to_point, expected tile_ranges) of one-tile splats in ``tiles``"""
  tw, th, ts = grid
  n = tiles.shape[0]
  depth = pc.few_depths(n, seed)
  f = Frame(n, pc.image_size(grid), ts, mapper, k_capacity, points7=pc.one_tile_splats(tiles, grid), depth=depth)
  f.project_count().map_raster()
  want_o2p, want_ranges = pc.expected_lists(tiles, omap.depth_key_bits(depth, False), tw * th)
  return f, want_o2p, want_ranges


def _assert_lists(f, K, want_o2p, want_ranges, label):
  assert f.counters[:3].tolist() == [K, K, 0], f"{label}: counters {f.counters[:3].tolist()}"
  assert np.array_equal(f.tile_ranges, want_ranges), f"{label}: tile_ranges"
  assert np.array_equal(f.overlap_to_point(K), want_o2p), f"{label}: overlap_to_point"


@pytest.mark.parametrize('mapper', list(MAPPERS))
@pytest.mark.parametrize('assignment', pc.ASSIGNMENTS)
@pytest.mark.parametrize('grid', list(pc.GRIDS))
def test_lists_at_chosen_k(grid, assignment, mapper):
  """K on every side of the keys-per-thread, wave and block boundaries of the range kernels, in the first / last tile,
  over all tiles and with empty tiles in between; k_capacity = K"""
  g = pc.GRIDS[grid]
  for K in pc.CHOSEN_K:
    tiles = pc.tile_assignment(assignment, K, g[0] * g[1])
    f, want_o2p, want_ranges = _run_chosen(g, tiles, MAPPERS[mapper], K, seed=K)
    _assert_lists(f, K, want_o2p, want_ranges, f"K {K}")


@pytest.mark.parametrize('mapper', list(MAPPERS))
def test_lists_on_a_grid_of_more_than_65536_tiles(mapper):
  """17 tile bits: three passes of the tile sort (6 + 6 + 5)"""
  g = pc.BIG_GRID
  K, num_tiles = 4097, g[0] * g[1]
  tiles = pc.tile_assignment('random_third', K, num_tiles)
  tiles[:4] = (num_tiles - 1, 0, 65536, 65535)
  f, want_o2p, want_ranges = _run_chosen(g, tiles, MAPPERS[mapper], K)
  _assert_lists(f, K, want_o2p, want_ranges, "big grid")


@pytest.mark.parametrize('mapper', list(MAPPERS))
@pytest.mark.parametrize('K', pc.CAPACITY_K)
def test_lists_do_not_depend_on_spare_capacity_and_overflow_is_flagged(K, mapper):
  g = pc.GRIDS['23x13_t8']
  tiles = pc.tile_assignment('random_third', K, g[0] * g[1])
  for capacity in (K, K + 65536):
    f, want_o2p, want_ranges = _run_chosen(g, tiles, MAPPERS[mapper], capacity)
    _assert_lists(f, K, want_o2p, want_ranges, f"capacity {capacity}")
  f, _, want_ranges = _run_chosen(g, tiles, MAPPERS[mapper], K - 1)
  assert f.counters[:3].tolist() == [K, 0, 1], "K above the capacity: live K 0, overflow flag set"
  assert not f.tile_ranges.any(), "on overflow every tile range is [0, 0)"
  assert not f.alpha.any().item(), "and nothing is blended"
