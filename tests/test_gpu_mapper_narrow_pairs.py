"""-m gpu: the direct-order mapper on narrow tile ids with 8-byte (depth key, point) payloads (ms_map_tiles_direct: the
launch sequence of the frame executor's direct branch, callable without a frame) against

  * the numpy oracle (oracle/mapper.py: one lexsort by (tile, depth bits, point index)),
  * map_to_tiles_strip(method='presort'), the second construction of the same lists on the device (gaussians sorted by
    depth, overlaps sorted by tile id: no kernel of the direct sequence behind its order), and
  * map_to_tiles_strip(method='direct'), the operator's wrapper of the same entry point: capacity exactly K, its own
    allocations and early returns.

Integer lists: overlap_to_point and tile_ranges must be IDENTICAL, no tolerance.  The scenes aim at the edges of the
narrow form: the 2-byte / 4-byte id switch at 65 536 tiles, the radix block edge (4096 pairs), runs at the class
boundaries of tile_sort.hip (1024 / 2560 / 5120) read as payload words only — a run of ONE entry must still be copied
out — the declined (bounded) path, ties, capacity above and below K, strips, and a float64 frame.  The mapper runs without an
image, so the 4096 x 4096 cases cost what their few thousand gaussians cost."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import mapper as omap
from taichi_splatting_amd import RasterConfig, _lib, frame, pad_to_tile
from taichi_splatting_amd.mapper.tile_mapper import map_to_tiles_strip
from taichi_splatting_amd.misc.renderer2d import project_gaussians2d
from taichi_splatting_amd.testing import random_2d_gaussians

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
THR = 1.0 / 255.0
UNTOUCHED = -7


def direct(p, depth, size, tile=16, depth16=False, rows=None, ndc=None, capacity=None, slack=37):
  """ms_tile_count -> ms_exclusive_scan_i32 -> ms_map_tiles_direct.  Returns (overlap_to_point [capacity], tile_ranges,
  counters [8], K); overlap_to_point is pre-filled with UNTOUCHED."""
  lib = _lib.load()
  dev = torch.device(DEV)
  stream = _lib.current_stream(dev)
  points = p.to(DEV).to(torch.float32).contiguous()
  depths = depth.to(DEV).reshape(-1).contiguous()
  v = points.shape[0]
  w_pad, h_pad = pad_to_tile(size, tile)
  tiles_high, tiles_wide = h_pad // tile, w_pad // tile
  row_begin, row_end = (0, tiles_high) if rows is None else rows
  counts = torch.empty((max(v, 1),), dtype=torch.int32, device=DEV)
  cum = torch.zeros((v + 1,), dtype=torch.int32, device=DEV)
  _lib.check(lib.ms_tile_count(points.data_ptr(), None, v, w_pad, h_pad, tile, THR, row_begin, row_end, counts.data_ptr(),
                               None, stream), "ms_tile_count")
  nb = ctypes.c_size_t(0)
  _lib.check(lib.ms_exclusive_scan_i32(None, v, None, None, None, ctypes.byref(nb), stream), "scan")
  tmp = torch.empty((max(nb.value, 1),), dtype=torch.uint8, device=DEV)
  _lib.check(lib.ms_exclusive_scan_i32(counts.data_ptr(), v, cum.data_ptr(), None, tmp.data_ptr(), ctypes.byref(nb), stream), "scan")
  k = int(cum[v])
  capacity = k + slack if capacity is None else capacity
  o2p = torch.full((max(capacity, 1),), UNTOUCHED, dtype=torch.int32, device=DEV)
  ranges = torch.full((tiles_high, tiles_wide, 2), -1, dtype=torch.int32, device=DEV)
  counters = torch.full((8,), -1, dtype=torch.int32, device=DEV)
  near, far = (0.0, 0.0) if ndc is None else ndc

  def call(scratch_ptr):
    return lib.ms_map_tiles_direct(points.data_ptr(), depths.data_ptr(), _lib.dtype_code(depths.dtype), cum.data_ptr(), v,
                                   w_pad, h_pad, tile, THR, row_begin, row_end, int(depth16), near, far, capacity,
                                   o2p.data_ptr(), ranges.data_ptr(), counters.data_ptr(), scratch_ptr, ctypes.byref(nb), stream)
  _lib.check(call(None), "ms_map_tiles_direct (size query)")
  scratch = torch.empty((max(nb.value, 1),), dtype=torch.uint8, device=DEV)
  _lib.check(call(scratch.data_ptr()), "ms_map_tiles_direct")
  torch.cuda.synchronize()
  return o2p, ranges, counters.tolist(), k


def check(p, depth, size, tile=16, depth16=False, rows=None, **kw):
  """the entry point == the oracle == the pre-sort construction == the operator's wrapper; returns (K, tile_ranges of
  the oracle)"""
  p, depth = p.to(torch.float32), depth.reshape(-1, 1)
  o2p, ranges, counters, k = direct(p, depth, size, tile, depth16, rows, **kw)
  want_o2p, want_ranges, _ = omap.map_to_tiles(p.numpy(), depth.to(torch.float32).numpy(), size, tile, THR, use_depth16=depth16,
                                               tile_rows=rows)
  assert counters[:3] == [k, k, 0], counters
  assert k == want_o2p.shape[0]
  assert np.array_equal(ranges.cpu().numpy(), want_ranges)
  bad = np.nonzero(o2p[:k].cpu().numpy() != want_o2p)[0]
  assert bad.size == 0, f"{bad.size} of {k} entries differ from the oracle, first at {int(bad[0])}"
  assert bool((o2p[k:] == UNTOUCHED).all())                       # nothing written past K
  cfg = RasterConfig(tile_size=tile, pixel_stride=(1, 1) if tile == 8 else (2, 2), alpha_threshold=THR)
  for method in ('presort', 'direct'):
    m_o2p, m_ranges = map_to_tiles_strip(p.to(DEV), depth.to(DEV), size, cfg, use_depth16=depth16, tile_rows=rows, method=method)
    assert torch.equal(m_ranges, ranges) and torch.equal(m_o2p, o2p[:k]), method
  return k, want_ranges


def one_tile_splats(tiles_xy, size_of_run, tile=16, seed=0):
  """Small splats that each overlap exactly ONE tile (1.5 px extent around the tile centre): run `size_of_run[j]` of them
  in tile `tiles_xy[j]`, shuffled, so that a tile's run is a scattered subset of the point indices."""
  gen = torch.Generator().manual_seed(seed)
  tile_of = torch.repeat_interleave(torch.arange(len(tiles_xy)), torch.as_tensor(size_of_run))
  tile_of = tile_of[torch.randperm(tile_of.numel(), generator=gen)]
  centre = (torch.as_tensor(tiles_xy, dtype=torch.float32)[tile_of] + 0.5) * tile
  n = tile_of.numel()
  p = torch.zeros((n, 7))
  p[:, 0:2] = centre + (torch.rand((n, 2), generator=gen) - 0.5) * 4.0
  p[:, 2] = 1.0
  p[:, 4:6] = 0.5
  p[:, 6] = 0.5
  return p, tile_of


def random_scene(n, size, scale, seed):
  torch.manual_seed(seed)
  g = random_2d_gaussians(n, size, scale_factor=scale, alpha_range=(0.2, 0.9))
  return project_gaussians2d(g), g.depths.reshape(-1).clone()


def test_small_random_scene_u16_ids():
  p, depth = random_scene(2000, (256, 192), 1.0, 1)
  k, _ = check(p, depth, (256, 192))
  assert k > 2000


def test_exactly_65536_tiles_uses_the_top_u16_id():
  size = (4096, 4096)
  p, depth = random_scene(3000, size, 0.2, 2)
  corners, _ = one_tile_splats([(0, 0), (255, 255)], [40, 40], seed=3)
  p, depth = torch.cat([p, corners]), torch.cat([depth, torch.rand(80)])
  _, ranges = check(p, depth, size)
  assert ranges.shape == (256, 256, 2)
  lengths = (ranges[..., 1] - ranges[..., 0]).reshape(-1)
  assert lengths[0] >= 40 and lengths[65535] >= 40


def test_more_than_65536_tiles_uses_u32_ids():
  size = (4112, 4096)                                             # 257 x 256 = 65 792 tiles, three radix passes
  p, depth = random_scene(3000, size, 0.2, 4)
  last_row, _ = one_tile_splats([(1, 255), (200, 255), (256, 255), (0, 255)], [30, 30, 30, 30], seed=5)
  p, depth = torch.cat([p, last_row]), torch.cat([depth, torch.rand(120)])
  _, ranges = check(p, depth, size)
  lengths = (ranges[..., 1] - ranges[..., 0]).reshape(-1)
  assert lengths.shape[0] == 65792 and lengths[65536] >= 30 and lengths[65791] >= 30 and lengths[65535] >= 30


def test_equal_depths_inside_a_tile_keep_ascending_point_index():
  p, depth = random_scene(6000, (192, 128), 3.0, 6)
  check(p, torch.full_like(depth, 0.25), (192, 128))
  # 96 depths, one per tile of the splat's centre: long runs of equal keys inside every tile next to other keys
  tile_depth = (torch.floor(p[:, 0] / 16) + 12 * torch.floor(p[:, 1] / 16)).clamp(0, 95) / 96 + 0.01
  check(p, tile_depth, (192, 128))
  o2p, got_ranges, _, _ = direct(p, torch.full_like(depth, 0.25), (192, 128))
  o2p, r = o2p.cpu().numpy(), got_ranges.cpu().numpy().reshape(-1, 2)
  assert all(np.all(np.diff(o2p[a:b]) > 0) for a, b in r)


def test_depth16_with_many_ties():
  p, depth = random_scene(6000, (256, 256), 2.0, 7)
  check(p, torch.floor(depth * 8) / 8 + 0.01, (256, 256), depth16=True)
  check(p, depth, (256, 256), depth16=True)


def test_runs_at_the_class_boundaries_of_the_tile_sort():
  runs = [1, 2, 1024, 1025, 2560, 2561, 5121]
  tiles = [(x, 0) for x in range(len(runs))]
  p, _ = one_tile_splats(tiles, runs, seed=8)
  torch.manual_seed(8)
  _, ranges = check(p, torch.rand(p.shape[0]), (16 * len(runs), 16))
  assert (ranges[0, :, 1] - ranges[0, :, 0]).tolist() == runs
  check(p, torch.full((p.shape[0],), 0.5), (16 * len(runs), 16))               # one key: every class copies its run out


def test_two_values_and_an_outlier_take_the_declined_path():
  # 2000 entries whose keys are two neighbouring floats, and ONE far below them: the monotone map puts the two values
  # into one bucket, the bucket sort declines the run and the long-run kernel takes it through the bounded radix path
  p, tile_of = one_tile_splats([(0, 0), (1, 0)], [2000, 300], seed=9)
  torch.manual_seed(9)
  depth = torch.where(torch.rand(p.shape[0]) < 0.5, torch.tensor(0.5), torch.nextafter(torch.tensor(0.5), torch.tensor(1.0)))
  depth[int((tile_of == 0).nonzero()[5])] = 1e-3
  _, ranges = check(p, depth, (32, 16))
  assert (ranges[0, :, 1] - ranges[0, :, 0]).tolist() == [2000, 300]


def test_no_overlaps_at_all():
  p = torch.tensor([[-500., -500., 1, 0, 2, 2, 0.5], [50., 30., 1, 0, 2, 2, 0.001], [9000., 20., 1, 0, 2, 2, 0.9]])
  o2p, ranges, counters, k = direct(p, torch.rand(3), (100, 60))
  assert k == 0 and counters[:3] == [0, 0, 0]
  assert int(ranges.abs().sum()) == 0 and bool((o2p == UNTOUCHED).all())
  o2p, ranges, counters, k = direct(p, torch.rand(3), (100, 60), capacity=0)
  assert counters[:3] == [0, 0, 0] and int(ranges.abs().sum()) == 0


@pytest.mark.parametrize('k', [1, 4096, 4097])
def test_radix_block_edge(k):
  tiles = [(x, y) for y in range(3) for x in range(5)]
  gen = torch.Generator().manual_seed(k)
  runs = torch.bincount(torch.randint(0, len(tiles), (k,), generator=gen), minlength=len(tiles)).tolist()
  p, _ = one_tile_splats(tiles, runs, seed=k)
  torch.manual_seed(k)
  depth = torch.rand(k)
  got_k, _ = check(p, depth, (80, 48), slack=0)                   # capacity == K exactly
  assert got_k == k
  check(p, depth, (80, 48), slack=5000)                           # capacity above K: idle blocks behind the live count


def test_capacity_below_k_writes_nothing_and_flags_the_overflow():
  p, depth = random_scene(2000, (256, 192), 1.0, 10)
  _, _, _, k = direct(p, depth, (256, 192))
  o2p, ranges, counters, _ = direct(p, depth, (256, 192), capacity=k - 1)
  assert counters[:3] == [k, 0, 1]
  assert bool((o2p == UNTOUCHED).all()) and int(ranges.abs().sum()) == 0


def test_a_strip_of_tile_rows():
  p, depth = random_scene(5000, (256, 192), 2.0, 11)
  k_all, _ = check(p, depth, (256, 192))
  total = 0
  for rows in ((0, 3), (3, 8), (8, 12)):
    k, ranges = check(p, depth, (256, 192), rows=rows)
    lengths = ranges[..., 1] - ranges[..., 0]
    assert int(lengths[:rows[0]].sum()) == 0 and int(lengths[rows[1]:].sum()) == 0 and int(lengths.sum()) == k
    total += k
  assert total == k_all


def test_float64_depths_and_ndc_keys():
  p, depth = random_scene(4000, (200, 144), 2.0, 12)
  check(p, depth.double(), (200, 144))
  # ndc keys are made inside the emit kernel from camera depths: against the pre-sort construction, whose first radix
  # pass makes them with the same function, depth_sort_key (the oracle takes ready keys)
  cam_depth = (0.2 + 50.0 * depth).double()
  cfg = RasterConfig(tile_size=16, alpha_threshold=THR)
  o2p, ranges, counters, k = direct(p, cam_depth, (200, 144), ndc=(0.1, 100.0))
  assert counters[:3] == [k, k, 0]
  for method in ('presort', 'direct'):                            # 'direct': the wrapper hands ndc_range on
    m_o2p, m_ranges = map_to_tiles_strip(p.to(DEV), cam_depth.reshape(-1, 1).to(DEV), (200, 144), cfg, ndc_range=(0.1, 100.0),
                                         method=method)
    assert torch.equal(m_ranges, ranges) and torch.equal(m_o2p, o2p[:k]), method


def test_a_float64_frame_on_the_direct_sequence():
  size, n = (200, 144), 4000
  p, depth = random_scene(n, size, 2.0, 13)
  cfg = RasterConfig(tile_size=16, alpha_threshold=THR)
  want_o2p, want_ranges, _ = omap.map_to_tiles(p.numpy(), depth.numpy(), size, 16, THR)
  pd, dd = p.to(DEV).double(), depth.to(DEV).double()
  features = torch.rand(n, 3, device=DEV, dtype=torch.float64)
  frame.release_caches()
  try:
    key = ('2d',) + frame._shape_key(torch.device(DEV), n, size, cfg, None, False)
    frame.shape_record(key, create=True).mapper = _lib.MAPPER_DIRECT
    state = frame.FrameState()
    frame._RasterizeFrameFunction.apply(pd, dd, features, size, cfg, False, state)
    state.settle()
    torch.cuda.synchronize()
    assert int(state.desc.mapper) == _lib.MAPPER_DIRECT and int(state.desc.dtype) == _lib.MS_F64
    k, live, overflow = state.counters()[:3].tolist()
    assert (k, live, overflow) == (want_o2p.shape[0], want_o2p.shape[0], 0)
    assert np.array_equal(state.tile_ranges().cpu().numpy().reshape(want_ranges.shape), want_ranges)
    assert np.array_equal(state.overlap_to_point()[:k].cpu().numpy(), want_o2p)
  finally:
    frame.release_caches()
