"""CPU conditions on the cases of tests/segment_cases.py, before a kernel is looked at (tests/test_gpu_raster_segments.py):
the lists have the stated runs, every listed splat is gate-stable at the case's own gate, every segment really blends
(or, for the saturating case, the oracle alone meets the cap on rows left out), the gradients are not zero, the float64
oracle is quick — and each property of the plan's contract, restated in segment_cases.plan_violations, can fail.

Observed here (float64 oracle, forward plus backward, seconds / largest image_weight):
  the tile-16 cases 0.2 / 0.78   edges8 0.1 / 0.78   edges32 0.5 / 0.23   deepest8 0.8 / 0.711   clamped8 0.8 / 0.708
  saturating16 0.2 / 1.0: 343 pixels saturate, at list positions 490 .. 1319 (median 706, 229 of them between 600 and 900);
  no row has a pair within 1e-4 of the saturation limit."""
import time

import numpy as np
import pytest
import torch

from oracle import raster as orast

from . import segment_cases as sc


@pytest.mark.parametrize('name', list(sc.CASES))
def test_case_lists_and_oracle_conditions(name):
  t0 = time.perf_counter()
  b = sc.build(name)
  built = time.perf_counter() - t0
  case, cfg = b.case, sc.config(b.case)
  runs = (b.ranges[:, 1] - b.ranges[:, 0]).tolist()
  assert tuple(runs) == case.runs
  assert b.o2p.shape[0] <= 66000 and b.o2p.shape[0] == max(case.runs) * len(case.runs)
  assert int(b.ranges.min()) >= 0 and int(b.ranges[:, 1].max()) <= b.o2p.shape[0]
  assert sc.effective_params(case.min_run, case.seg_len, case.tile) == case.expect
  # every tile's list names each splat once, and only splats centred in that tile (the scene is confined)
  tw, _ = sc.tiles_of(case.size, case.tile)
  for t, (s, e) in enumerate(b.ranges.tolist()):
    ids = b.o2p[s:e].long()
    assert ids.unique().numel() == ids.numel()
    centre = (b.p[ids, :2] / case.tile).floor().long()
    assert bool((centre[:, 0] + centre[:, 1] * tw == t).all()), t
  # gate-stable at the case's own gate, on the shortened lists
  margin = orast.gate_margin(b.p.double(), b.ranges, b.o2p, case.size, cfg)
  listed = b.listed
  assert int(listed.sum()) == sum(case.runs)
  assert float(margin[listed].min()) > sc.STABLE_MARGIN and bool(torch.isinf(margin[~listed]).all())
  assert case.alpha_range[0] > cfg.alpha_threshold                     # opacities sit just above the gate
  assert b.stable_share > 0.99

  t0 = time.perf_counter()
  sc.oracle.cache_clear()
  o = sc.oracle(name)
  seconds = time.perf_counter() - t0
  print(f"{name}: lists {built:.2f} s, float64 oracle forward + backward {seconds:.2f} s, largest image_weight "
        f"{float(o['alpha'].max()):.4f}, gate-stable share of the pool {b.stable_share:.4f}")
  assert seconds < 5.0
  for key in ('grad_points', 'grad_features', 'heuristics', 'visibility'):
    assert float(o[key].abs().max()) > 0, key
    assert float(o[key][~listed].abs().max()) == 0 if bool((~listed).any()) else True
  if case.saturating:
    rows = sc.compared_rows(name)
    left_out = 1.0 - float(rows[listed].float().mean())
    first = sc.first_saturated_entry(name)
    sat = first[first >= 0]
    print(f"{name}: {100 * left_out:.3f} % of the listed rows left out; {sat.numel()} pixels saturate, first dropped entry "
          f"{int(sat.min())} .. {int(sat.max())}, median {int(sat.median())}")
    assert left_out <= sc.LEFT_OUT_CAP
    # pixels of the long tiles saturate inside a LATER segment (the second of 512): behind entry 600, before entry 900
    assert int(((sat >= 600) & (sat <= 900)).sum()) >= 100 and 600 <= int(sat.median()) <= 900
    long_tiles = [t for t, r in enumerate(case.runs) if r > 900]
    th = sc.tiles_of(case.size, case.tile)[1]
    per_tile = first.reshape(th, case.tile, tw, case.tile).permute(0, 2, 1, 3).reshape(th * tw, -1)
    for t in long_tiles:
      assert int(((per_tile[t] >= 600) & (per_tile[t] <= 900)).sum()) > 0, t
  else:
    assert 0.05 < float(o['alpha'].max()) < 0.999                      # every segment really blends


def test_window_case_has_cut_and_uncut_tiles_in_and_above_the_window():
  case = sc.CASES['window16']
  assert sorted(case.runs) == sorted(sc.EDGE_RUNS)
  tw, th = sc.tiles_of(case.size, case.tile)
  row0, rest = case.runs[:tw], case.runs[tw:]
  for part in (row0, rest):
    assert any(r > case.expect[0] for r in part) and any(0 < r <= case.expect[0] for r in part)
  # the oracle of the window leaves the splats of tile row 0 alone
  b = sc.build('window16')
  o = sc.oracle('window16', tile_rows=(1, th))
  above = b.p[:, 1] < case.tile
  assert float(o['grad_points'][above].abs().max()) == 0 and float(o['grad_points'][~above & b.listed].abs().max()) > 0
  assert float(o['image'][:case.tile].abs().max()) == 0


def expected_plan(name):
  """{tile: segment lengths} and the (tile, begin, end) items of a case, from segment_cases.expected_segments"""
  b = sc.build(name)
  segments, items = {}, []
  for t, (s, e) in enumerate(b.ranges.tolist()):
    lengths = sc.expected_segments(e - s, *b.case.expect)
    if lengths:
      segments[t] = lengths
      edges = np.concatenate([[s], s + np.cumsum(lengths)])
      items += [(t, int(edges[i]), int(edges[i + 1])) for i in range(len(lengths))]
  return b, segments, items


@pytest.mark.parametrize('name', list(sc.CASES))
def test_the_table_reaches_its_edges(name):
  """the plan the kernels make of each case (segment_cases.expected_segments) keeps the restated contract and has the
  shape the case is in the table for"""
  b, segments, items = expected_plan(name)
  assert sc.plan_violations(items, b.ranges, *b.case.expect) == []
  by_run = {b.case.runs[t]: lengths for t, lengths in segments.items()}
  cut = sorted(by_run)
  if name in ('edges16', 'edges8', 'saturating16', 'window16'):
    assert cut == [513, 768, 1024, 1025, 1279, 1400]
    assert by_run[513] == [512, 1] and by_run[1024] == [512, 512] and by_run[1025] == [512, 512, 1] and by_run[1400] == [512, 512, 376]
  elif name == 'edges32':
    assert cut == [513, 1024, 1025, 1400] and by_run[513] == [512, 1] and by_run[1025] == [512, 512, 1]
  elif name == 'short_segments16':
    assert cut == [1025, 1279, 1400] and by_run[1025] == [256, 256, 256, 256, 1] and len(by_run[1400]) == 6
  elif name == 'one_segment16':
    # runs of 257 .. 1024 entries: long tiles of ONE item (the contract leaves nothing else: an item that is not the last
    # has at least 1024 entries); 1025 entries: a full segment and a last segment of one entry
    assert cut == [511, 512, 513, 768, 1024, 1025, 1279, 1400]
    assert all(by_run[r] == [r] for r in (511, 512, 513, 768, 1024))
    assert by_run[1025] == [1024, 1] and by_run[1400] == [1024, 376]
  elif name == 'raised16':
    assert cut == [511, 512, 513, 768, 1024, 1025, 1279, 1400] and by_run[511] == [256, 255] and by_run[513] == [256, 256, 1]
  elif name == 'deepest8':
    assert by_run[65536] == [256] * 256
  elif name == 'clamped8':
    assert by_run[65537] == [512] * 128 + [1]                  # 257 segments of 256 do not fit: the clamp doubles the length
  else:
    raise AssertionError(name)
  assert len(items) <= sc.carve(b.o2p.shape[0], b.case.tile, *b.case.expect)['item_cap']
  assert len(segments) <= sc.carve(b.o2p.shape[0], b.case.tile, *b.case.expect)['long_cap']


def test_expected_segments_keep_the_contract_for_every_run():
  """every run of 0 .. 3000 entries and a few long ones, at the parameter pairs of the table and the defaults"""
  for min_run, seg_len in ((512, 512), (1024, 256), (256, 1024), (256, 256), (16384, 1024), (16384, 4096)):
    for run in list(range(0, 3001)) + [16384, 16385, 20000, 65535, 65536, 65537, 262144, 262145, 1 << 20, (1 << 24) + 1]:
      lengths = sc.expected_segments(run, min_run, seg_len)
      edges = np.concatenate([[7], 7 + np.cumsum(lengths)]).astype(np.int64)
      items = [(0, int(edges[i]), int(edges[i + 1])) for i in range(len(lengths))]
      assert sc.plan_violations(items, np.array([[7, 7 + run]]), min_run, seg_len) == [], (min_run, seg_len, run)
      assert len(lengths) <= min(256, run // seg_len + 1)                   # what the scratch block's item capacity counts on


def test_parameter_rules():
  assert sc.effective_params(0, 0, 16) == (16384, 1024) and sc.effective_params(0, 0, 32) == (16384, 4096)
  assert sc.effective_params(0, 0, 8) == (16384, 1024)
  assert sc.effective_params(100, 1, 16) == (256, 256) and sc.effective_params(255, 255, 16) == (256, 256)
  assert sc.effective_params(256, 256, 16) == (256, 256) and sc.effective_params(257, 257, 16) == (257, 512)
  assert sc.effective_params(512, 1000, 32) == (512, 1024)


def test_carve_is_the_librarys_scratch_size():
  """the reader's restatement of split_scratch_carve gives the size ms_raster_split_scratch_bytes reports (host code), for
  every case's k_capacity, tile size and PASSED parameters — the parameter rules included"""
  from taichi_splatting_amd import _lib
  lib = _lib.load()
  for case in sc.CASES.values():
    for k in (max(case.runs) * len(case.runs), 1, 255, 256, 65537):
      want = lib.ms_raster_split_scratch_bytes(k, case.tile, case.min_run, case.seg_len)
      assert sc.carve(k, case.tile, *case.expect)['bytes'] == want, (case.name, k)
  for tile in (8, 16, 32):
    assert sc.carve(100000, tile, *sc.effective_params(0, 0, tile))['bytes'] == lib.ms_raster_split_scratch_bytes(100000, tile, 0, 0)


# ---- the restated contract on hand-made plans: one plan that keeps it, one broken plan per property -----------------------
RANGES = np.array([[0, 512], [600, 1113], [1200, 2225], [3000, 3000]])          # runs 512, 513, 1025, 0
GOOD = [(1, 600, 1112), (1, 1112, 1113), (2, 1200, 1712), (2, 1712, 2224), (2, 2224, 2225)]


def violated(items, ranges=RANGES, min_run=512, seg_len=512, **kw):
  return sorted({v[0] for v in sc.plan_violations(items, ranges, min_run, seg_len, **kw)})


def test_a_plan_that_keeps_the_contract():
  assert violated(GOOD) == []
  assert violated(list(reversed(GOOD))) == []                                       # the item order is not part of it
  assert violated([(2, 1200, 2224), (2, 2224, 2225)], min_run=513, seg_len=1024) == []
  assert violated([(0, 0, 512), (1, 600, 1113), (2, 1200, 2225)], min_run=256, seg_len=1024) == []   # one item per long tile
  many = [(0, 256 * i, 256 * (i + 1)) for i in range(256)]
  assert violated(many, ranges=np.array([[0, 65536]]), min_run=256, seg_len=256) == []
  # a window of tile rows: tiles outside it have no items however long their runs
  assert violated([g for g in GOOD if g[0] == 2], tile_rows=(1, 2), tiles_wide=2) == []


def test_each_property_can_fail():
  # cut: a run of exactly min_run entries is cut; a run of min_run + 1 is not; a tile outside the window is
  assert violated(GOOD + [(0, 0, 512)]) == ['cut']
  assert violated([g for g in GOOD if g[0] != 1]) == ['cut']
  assert violated(GOOD, tile_rows=(1, 2), tiles_wide=2) == ['cut']
  assert violated(GOOD + [(7, 0, 512)]) == ['cut']
  # covers: a gap, an overlap, a short end, an early start, an empty item
  assert violated([(1, 600, 1112), (2, 1200, 1712), (2, 1712, 2224), (2, 2224, 2225)]) == ['covers']
  assert violated([g for g in GOOD if g[0] == 1] + [(2, 1200, 1712), (2, 1711, 2223), (2, 2223, 2225)]) == ['covers']
  assert violated([g for g in GOOD if g[0] == 1] + [(2, 1200, 1712), (2, 1712, 2224), (2, 2224, 2224)]) == ['covers']
  assert violated([g for g in GOOD if g[0] == 1] + [(2, 1199, 1711), (2, 1711, 2223), (2, 2223, 2225)]) == ['covers']
  # length: unequal, not a multiple of 256, shorter than seg_len, a last item longer than the others
  tile1 = [g for g in GOOD if g[0] == 1]
  assert violated(tile1 + [(2, 1200, 1456), (2, 1456, 2224), (2, 2224, 2225)], seg_len=256) == ['length']
  assert violated(tile1 + [(2, 1200, 1700), (2, 1700, 2200), (2, 2200, 2225)], seg_len=256) == ['length']
  assert violated(tile1 + [(2, 1200, 1968), (2, 1968, 2225)], seg_len=1024) == ['length']
  assert violated(tile1 + [(2, 1200, 1456), (2, 1456, 2225)], seg_len=256) == ['length']
  # count: 257 items
  many = [(0, 256 * i, 256 * (i + 1)) for i in range(257)]
  assert violated(many, ranges=np.array([[0, 65792]]), min_run=256, seg_len=256) == ['count']


def test_reader_and_plan_check_on_a_hand_made_block():
  """read_plan on a block laid out by hand the way split_scratch_carve documents it, items of the two tiles interleaved
  out of tile order (their order comes from atomics), and check_plan's count conditions"""
  k, tile, min_run, seg_len = 2225, 16, 512, 512
  c = sc.carve(k, tile, min_run, seg_len)
  assert (c['long_cap'], c['item_cap']) == (5, 10) and (c['long_tiles'], c['items'], c['state']) == (256, 512, 768)
  raw = np.zeros(c['bytes'], dtype=np.uint8)
  words = raw.view(np.int32)
  items = [(2, 1200, 1712, 0), (2, 1712, 2224, 0), (2, 2224, 2225, 0), (1, 600, 1112, 3), (1, 1112, 1113, 3)]
  longs = [(2, 0, 3, 0), (1, 3, 2, 0)]
  words[:4] = (5, 2, 0, 0)
  words[c['long_tiles'] // 4:c['long_tiles'] // 4 + 8] = np.array(longs).reshape(-1)
  words[c['items'] // 4:c['items'] // 4 + 20] = np.array(items).reshape(-1)
  counts, long_tiles, got = sc.read_plan(torch.from_numpy(raw), k, tile, min_run, seg_len)
  assert counts.tolist() == [5, 2, 0, 0] and long_tiles.tolist() == [list(r) for r in longs] and got.tolist() == [list(r) for r in items]
  assert sc.check_plan(counts, long_tiles, got, RANGES, min_run, seg_len) == {2: [512, 512, 1], 1: [512, 1]}
  for broken in ((5, 2, 1, 0), (5, 3, 0, 0), (4, 2, 0, 0)):
    with pytest.raises(AssertionError):
      sc.check_plan(np.array(broken), long_tiles, got, RANGES, min_run, seg_len)
