"""-m gpu: the long-run segment kernels (ms_raster_fwd_split / ms_raster_bwd_moments_split; csrc/raster_fast.hip
split_plan_kernel, split_combine_kernel and the SEGS instances, csrc/raster_bwd_scan.hip's SEGS instance) at the edges of
their PLAN, against the float64 oracle, on lists with chosen run lengths (tests/segment_cases.py; the CPU conditions on
the cases are tests/test_segment_cases_host.py's):

a. every case of the table against the oracle: image and image_weight to 1e-4 on every pixel, visibility to 1e-4 of its
   largest entry, every gradient row to 1e-4 of the largest gradient (the project's float32 raster contract,
   tests/test_gpu_round6.py) — runs of exactly min_run entries next to min_run + 1 (a last segment of ONE entry), exact
   multiples of the segment length and one more, seg_len below and above min_run (many short segments; long tiles of one
   segment), parameters raised to 256, 256 segments in one tile and the clamp behind it, empty / short / uncut / cut tiles
   in one launch, saturation inside a later segment;
b. the plan the device left in the scratch block keeps the documented contract (segment_cases.plan_violations), its counts
   are right, and it has the shape the case is in the table for;
c. uncut tiles of a split launch are bit for bit the per-tile kernel's;
d. a tile-row window that starts at row 1: nothing outside the window is written, splats of row 0 keep zero rows;
e. deterministic commits on a mixed plan: bit-equal int64 rows whatever the plan's item order;
f. the frame executor on a scene that makes its own mixed lists.

Each test prints its figures (pytest -s): "segment figures", "segment plan" and report_rows' "parity rows"."""
import functools
import json

import numpy as np
import pytest
import torch

from oracle import raster as orast
from taichi_splatting_amd import _lib, frame, rasterize

from . import segment_cases as sc
from .test_gpu_round6 import TOL, cfg_for, finalize, oracle_pair, report_rows, split_forward_backward

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def cfg_of(case, visibility=False, heuristics=False):
  gate = {} if case.alpha_threshold is None else dict(alpha_threshold=case.alpha_threshold)
  cfg = cfg_for(case.tile, compute_visibility=visibility, compute_point_heuristic=heuristics, **gate)
  assert cfg == sc.config(case, compute_visibility=visibility, compute_point_heuristic=heuristics)
  return cfg


@functools.lru_cache(maxsize=None)
def device_lists(name):
  """(p, f, o2p, ranges, G) of a case on the device"""
  b = sc.build(name)
  return tuple(t.to(DEV).contiguous() for t in (b.p, b.f, b.o2p, b.ranges, sc.grad_image(b.case.size)))


@functools.lru_cache(maxsize=None)
def oracle_of(name):
  """(image, alpha, visibility, d gaussians2d, d features, heuristics) in float64, once per case (shared: read only)"""
  p, f, o2p, ranges, G = device_lists(name)
  case = sc.CASES[name]
  return oracle_pair(p, f, ranges, o2p, case.size, cfg_of(case), G)


def figures(what, **values):
  print('segment figures:', json.dumps({"what": what, **{k: float(v) for k, v in values.items()}}))


def check_against_oracle(what, name, cfg, image, alpha, vis, gp, gf, heur, oracle=None, pixel_rows=None):
  """§a: every pixel, every visibility entry, every gradient row.  Saturating cases: gradient rows with a pair within
  1e-4 of the backward's saturation limit are left out (their oracle rows are put in their place, so that report_rows
  names the rows it lists by their real index and scales by the largest gradient of ALL rows: the host test caps the
  share left out and finds none in this draw)."""
  p, f, o2p, ranges, G = device_lists(name)
  case = sc.CASES[name]
  img_o, a_o, vis_o, gp_o, gf_o, heur_o = oracle_of(name) if oracle is None else oracle
  rows = slice(None) if pixel_rows is None else slice(*pixel_rows)
  fig = dict(image=(image.cpu().double() - img_o)[rows].abs().max(), weight=(alpha.cpu().double() - a_o)[rows].abs().max())
  if vis is not None:
    fig['visibility'] = (vis.cpu().double() - vis_o).abs().max() / vis_o.max()
  keep = sc.compared_rows(name)

  def held(got, want):
    return got if keep is None else torch.where(keep[:, None], got.detach().cpu().double(), want)
  fig['d_gaussians2d'] = report_rows(what + " d gaussians2d", held(gp, gp_o), gp_o, p, ranges, o2p, case.size, cfg)['largest']
  fig['d_features'] = report_rows(what + " d features", held(gf, gf_o), gf_o, p, ranges, o2p, case.size, cfg)['largest']
  if heur is not None:
    fig['heuristics'] = report_rows(what + " heuristics", held(heur, heur_o), heur_o, p, ranges, o2p, case.size, cfg)['largest']
  figures(what, **fig)
  assert bool(torch.isfinite(image[rows]).all()) and bool(torch.isfinite(alpha[rows]).all())
  assert float(fig['image']) < TOL and float(fig['weight']) < TOL, fig
  if vis is not None:
    assert float(fig['visibility']) < TOL, fig
  # splats no list names: nothing may have been committed to their rows
  unlisted = ~sc.build(name).listed.to(DEV)
  if bool(unlisted.any()):
    assert float(gp[unlisted].abs().max()) == 0 and float(gf[unlisted].abs().max()) == 0
  return fig


def run_split(name, cfg, tile_rows=None, backward=True, deterministic=0, fixed_exp=None):
  """ms_raster_fwd_split [+ ms_raster_bwd_moments_split + ms_raster_moments_finalize] on a tile-row window, image and
  weight pre-filled with NaN; also returns a CPU copy of the scratch block's plan taken behind the forward (what
  tests/test_gpu_round6.py's split_forward_backward does for the full window, without handing the block out)"""
  lib = _lib.load()
  p, f, o2p, ranges, G = device_lists(name)
  case = sc.CASES[name]
  (w, h), tile, n, k = case.size, case.tile, p.shape[0], o2p.shape[0]
  th = sc.tiles_of(case.size, tile)[1]
  r0, r1 = (0, th) if tile_rows is None else tile_rows
  cfg_c, stream = _lib.raster_config_c(cfg), _lib.current_stream(torch.device(DEV))
  nbytes = lib.ms_raster_split_scratch_bytes(k, tile, case.min_run, case.seg_len)
  carve = sc.carve(k, tile, *case.expect)
  assert nbytes == carve['bytes']
  scratch = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
  image, alpha = torch.full((h, w, 3), float('nan'), device=DEV), torch.full((h, w), float('nan'), device=DEV)
  vis = torch.zeros(n, device=DEV) if cfg.compute_visibility else None
  _lib.check(lib.ms_raster_fwd_split(p.data_ptr(), f.data_ptr(), ranges.data_ptr(), o2p.data_ptr(), k, w, h, cfg_c,
                                     image.data_ptr(), alpha.data_ptr(), _lib.ptr(vis), scratch.data_ptr(), case.min_run,
                                     case.seg_len, r0, r1, stream), "fwd split")
  out = dict(image=image, alpha=alpha, vis=vis, plan=sc.read_plan(scratch[:carve['state']].cpu(), k, tile, *case.expect))
  if backward:
    mom = torch.zeros((n, _lib.MOMENT_ROW), dtype=torch.int64 if deterministic else torch.float32, device=DEV)
    _lib.check(lib.ms_raster_bwd_moments_split(p.data_ptr(), f.data_ptr(), ranges.data_ptr(), o2p.data_ptr(), k, image.data_ptr(),
                                               G.data_ptr(), w, h, cfg_c, mom.data_ptr(), deterministic, _lib.ptr(fixed_exp),
                                               scratch.data_ptr(), case.min_run, case.seg_len, r0, r1, stream), "bwd split")
    out['mom'] = mom
    out['gp'], out['gf'], out['heur'] = finalize(lib, p, mom, cfg.compute_point_heuristic, stream, deterministic, fixed_exp)
  return out


# ---- a. every case against the oracle -------------------------------------------------------------------------------------
ORACLE_RUNS = [('edges16', True, False), ('edges16', False, True), ('edges16', False, False)] + \
  [(n, sc.CASES[n].visibility, sc.CASES[n].heuristics) for n in sc.TABLE if n != 'edges16']


@pytest.mark.parametrize('name,visibility,heuristics', ORACLE_RUNS)
def test_segment_plan_edges_vs_oracle(name, visibility, heuristics):
  lib, case = _lib.load(), sc.CASES[name]
  cfg = cfg_of(case, visibility, heuristics)
  p, f, o2p, ranges, G = device_lists(name)
  assert tuple((ranges[:, 1] - ranges[:, 0]).tolist()) == case.runs
  image, alpha, vis, gp, gf, heur, counts = split_forward_backward(lib, p, f, o2p, ranges, case.size, cfg, G, case.min_run,
                                                                   case.seg_len, k_capacity=o2p.shape[0])
  long_runs = sum(r > case.expect[0] for r in case.runs)
  assert int(counts[2]) == 0 and int(counts[1]) == long_runs > 0, counts[:3]
  a_o = oracle_of(name)[1]
  assert float(a_o.max()) > 0.9999 if case.saturating else 0.05 < float(a_o.max()) < 0.999
  what = f"segment edges {name}" + (" +vis" if visibility else "") + (" +heur" if heuristics else "")
  check_against_oracle(what, name, cfg, image, alpha, vis, gp, gf, heur)


# ---- b. the device's plan -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(sc.TABLE))
def test_device_plan_keeps_the_contract(name):
  case = sc.CASES[name]
  b = sc.build(name)
  counts, long_tiles, items = run_split(name, cfg_of(case), backward=False)['plan']
  segments = sc.check_plan(counts, long_tiles, items, b.ranges, *case.expect)
  by_run = {case.runs[t]: lengths for t, lengths in segments.items()}
  shortest = min(min(v) for v in segments.values())
  print('segment plan:', json.dumps({"case": name, "passed": [case.min_run, case.seg_len], "acts_as": list(case.expect),
                                     "long_tiles": int(counts[1]), "items": int(counts[0]), "shortest_segment": shortest,
                                     "most_items": max(len(v) for v in segments.values()),
                                     "segments_by_run": {str(r): (f"{len(v) - 1} x {v[0]} + {v[-1]}" if len(v) > 4 else v) for r, v in sorted(by_run.items())}}))
  uncut = [r for t, r in enumerate(case.runs) if t not in segments]
  # non-vacuity, from the device's plan
  if name in ('edges16', 'saturating16'):
    assert by_run[513] == [512, 1] and by_run[1025][-1] == 1 and 512 in uncut
  if name == 'one_segment16':
    assert any(len(v) == 1 for v in segments.values()) and all(by_run[r] == [r] for r in (511, 512, 513, 768, 1024))
  if name == 'short_segments16':
    assert by_run[1025] == [256, 256, 256, 256, 1] and 1024 in uncut
  if name == 'deepest8':
    assert [len(v) for v in segments.values()] == [256] and set(by_run[65536]) == {256}
  if name == 'clamped8':
    assert len(by_run[65537]) <= 256 and by_run[65537][-1] == 1
  if name == 'raised16':
    assert sorted(by_run) == [511, 512, 513, 768, 1024, 1025, 1279, 1400] and sorted(uncut) == [0, 1, 255]
  # and it is the plan the host test derived the table's edges from
  assert segments == {t: sc.expected_segments(r, *case.expect) for t, r in enumerate(case.runs) if r > case.expect[0]}


# ---- c. uncut tiles are the per-tile kernel's -----------------------------------------------------------------------------
def test_uncut_tiles_of_a_split_launch_are_the_per_tile_kernels():
  name = 'edges16'
  lib, case = _lib.load(), sc.CASES[name]
  cfg = cfg_of(case)
  p, f, o2p, ranges, _ = device_lists(name)
  out = run_split(name, cfg, backward=False)
  (w, h), tile = case.size, case.tile
  tw, th = sc.tiles_of(case.size, tile)
  image, alpha = torch.full((h, w, 3), float('nan'), device=DEV), torch.full((h, w), float('nan'), device=DEV)
  _lib.check(lib.ms_raster_fwd(p.data_ptr(), f.data_ptr(), ranges.data_ptr(), o2p.data_ptr(), w, h, 3, _lib.raster_config_c(cfg),
                               image.data_ptr(), alpha.data_ptr(), None, 0, th, _lib.dtype_code(torch.float32),
                               _lib.current_stream(torch.device(DEV))), "fwd")
  cut_tiles = {int(t) for t in out['plan'][1][:, 0]}
  assert 0 < len(cut_tiles) < tw * th
  cut = torch.zeros((h, w), dtype=torch.bool, device=DEV)
  for t in cut_tiles:
    cut[(t // tw) * tile:(t // tw + 1) * tile, (t % tw) * tile:(t % tw + 1) * tile] = True
  assert torch.equal(out['image'][~cut], image[~cut]) and torch.equal(out['alpha'][~cut], alpha[~cut])
  assert not bool(torch.isnan(out['image']).any()) and float(image[~cut].max()) > 0
  figures("edges16 split launch vs per-tile kernel, cut tiles (not asserted)",
          image=(out['image'] - image)[cut].abs().max(), weight=(out['alpha'] - alpha)[cut].abs().max())


# ---- d. a window that starts at tile row 1 --------------------------------------------------------------------------------
def test_window_from_tile_row_one_vs_oracle():
  name = 'window16'
  case, b = sc.CASES[name], sc.build(name)
  cfg = cfg_of(case, heuristics=True)
  p, f, o2p, ranges, G = device_lists(name)
  tw, th = sc.tiles_of(case.size, case.tile)
  window = (1, th)
  out = run_split(name, cfg, tile_rows=window)
  segments = sc.check_plan(*out['plan'], b.ranges, *case.expect, tile_rows=window, tiles_wide=tw)
  in_window = [r for t, r in enumerate(case.runs) if t >= tw]
  assert len(segments) == sum(r > 512 for r in in_window) and any(0 < r <= 512 for r in in_window)
  assert any(r > 512 for r in case.runs[:tw]) and any(0 < r <= 512 for r in case.runs[:tw])     # row 0 has both kinds too
  first = case.tile                                                                              # first pixel row of the window
  assert bool(torch.isnan(out['image'][:first]).all()) and bool(torch.isnan(out['alpha'][:first]).all())
  p64, f64 = b.p.double(), b.f.double()
  img_o, a_o, vis_o = orast.forward(p64, f64, b.ranges, b.o2p, case.size, cfg, tile_rows=window)
  gp_o, gf_o, heur_o = orast.backward(p64, f64, b.ranges, b.o2p, img_o, G.cpu().double(), case.size, cfg, tile_rows=window)
  check_against_oracle("window rows 1..2 of window16", name, cfg, out['image'], out['alpha'], None, out['gp'], out['gf'], out['heur'],
                       oracle=(img_o, a_o, vis_o, gp_o, gf_o, heur_o), pixel_rows=(first, None))
  above = (b.p[:, 1] < case.tile).to(DEV)                       # confined: seen from tile row 0 only
  assert int(above.sum()) > 0 and float(out['mom'][above].abs().max()) == 0.0
  assert float(out['mom'][~above].abs().max()) > 0


# ---- e. deterministic mode on a mixed plan --------------------------------------------------------------------------------
def test_deterministic_rows_on_a_mixed_plan():
  name = 'edges16'
  lib, case = _lib.load(), sc.CASES[name]
  cfg = cfg_of(case, heuristics=True)
  p, f, o2p, ranges, G = device_lists(name)
  exps = _lib.fixed_point_exponents(G)
  rows, outs = [], []
  for _ in range(2):
    outs.append(split_forward_backward(lib, p, f, o2p, ranges, case.size, cfg, G, case.min_run, case.seg_len,
                                       k_capacity=o2p.shape[0], deterministic=1, fixed_exp=exps, rows_out=rows))
  assert rows[0].dtype == torch.int64 and torch.equal(rows[0], rows[1]) and int(rows[0].abs().max()) > 2 ** 30
  for a, c in zip(outs[0][3:6], outs[1][3:6]):
    assert torch.equal(a, c)
  image, alpha, vis, gp, gf, heur, counts = outs[0]
  assert int(counts[2]) == 0 and 0 < int(counts[1]) < len(case.runs)
  check_against_oracle("edges16 deterministic", name, cfg, image, alpha, vis, gp, gf, heur)


# ---- f. through the frame executor ----------------------------------------------------------------------------------------
def test_frame_executor_on_mixed_lists_vs_oracle():
  """rasterize() with the segment launches switched on (frame.set_split_policy) on a scene whose own lists mix tiles of
  1400 (cut), 300 (uncut) and no entries: image and both 2D gradients against the oracle on the frame's lists"""
  tile, size = sc.FRAME_TILE, sc.FRAME_SIZE
  cfg = cfg_for(tile)
  p, depth, f = (t.to(DEV).contiguous() for t in sc.frame_scene())
  depth = depth.reshape(-1, 1)
  G = sc.grad_image(size, seed=4).to(DEV)
  states = []

  class Recording(frame.FrameState):
    def __init__(self):
      super().__init__()
      states.append(self)
  original = frame.FrameState
  frame.release_caches()
  frame.set_split_policy(min_run=512, seg_len=512, always=True)
  frame.FrameState = Recording
  try:
    pg, fg = p.clone().requires_grad_(True), f.clone().requires_grad_(True)
    out = rasterize(pg, depth, fg, size, cfg)
    (out.image * G).sum().backward()
    torch.cuda.synchronize()
    st = states[-1]
    assert int(st.desc.split_long_runs) == 512 and int(st.desc.split_seg_len) == 512
    off = st.layout.split_scratch
    counts = st.keep_k[off:off + 16].view(torch.int32).cpu()
    k = int(st.counters()[0])
    ranges, o2p = st.tile_ranges().reshape(-1, 2).clone(), st.overlap_to_point()[:k].clone()
  finally:
    frame.FrameState = original
    frame.set_split_policy()
    frame.release_caches()
  runs = (ranges[:, 1] - ranges[:, 0]).cpu()
  assert tuple(runs.tolist()) == sc.FRAME_COUNTS and k == sum(sc.FRAME_COUNTS)           # the frame made the mixed lists
  nonempty = int((runs > 0).sum())
  assert int(counts[2]) == 0 and 0 < int(counts[1]) < nonempty and int(counts[1]) == int((runs > 512).sum()), counts[:3]
  assert int(counts[0]) == 3 * int(counts[1])
  img_o, a_o, _, gp_o, gf_o, _ = oracle_pair(p, f, ranges, o2p, size, cfg, G)
  assert 0.05 < float(a_o.max()) < 0.999
  fig = dict(image=(out.image.detach().cpu().double() - img_o).abs().max(), weight=(out.image_weight.cpu().double() - a_o).abs().max())
  fig['d_gaussians2d'] = report_rows("frame executor mixed lists, d gaussians2d", pg.grad, gp_o, p, ranges, o2p, size, cfg)['largest']
  fig['d_features'] = report_rows("frame executor mixed lists, d features", fg.grad, gf_o, p, ranges, o2p, size, cfg)['largest']
  figures("frame executor mixed lists", **fig)
  assert float(fig['image']) < TOL and float(fig['weight']) < TOL, fig
