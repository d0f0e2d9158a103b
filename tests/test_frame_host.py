"""CPU tests of the frame executor's host side (no kernels run): the per-shape policy record, the settle bookkeeping of a
frame state, the switches, the shared identity index list, the parked collector, the layout query."""
import ctypes
import gc

import numpy as np
import pytest
import torch

from taichi_splatting_amd import RasterConfig, _lib, frame

SPLIT_DEFAULTS = (True, False, 0, 0)        # SPLIT_LONG_RUNS, SPLIT_ALWAYS, SPLIT_MIN_RUN, SPLIT_SEG_LEN


@pytest.fixture
def words(monkeypatch):
  """stand-in for the pinned run words (pinning needs a device): the words handed out, in order"""
  made = []

  def make():
    t = torch.zeros((1,), dtype=torch.int32)
    made.append(t)
    return t, t.numpy()
  monkeypatch.setattr(frame, 'pinned_word', make)
  return made


def test_first_frame_of_a_shape_plans_presort_with_segments_then_what_was_observed(words):
  rec = frame.ShapeRecord()
  n = 1000
  capacity, mapper, split, seg_len, run_ptr = rec.plan(False, *SPLIT_DEFAULTS)
  assert (capacity, mapper, split, seg_len) == (0, _lib.MAPPER_PRESORT, 1, 0)
  assert len(words) == 1 and run_ptr == words[0].data_ptr()
  assert rec.plan(False, *SPLIT_DEFAULTS)[1:3] == (_lib.MAPPER_PRESORT, 1) and len(words) == 1     # still nothing observed
  # few overlaps per gaussian: the direct sequence without the segment launches from the next frame on
  rec.observe(int(frame.DIRECT_BELOW * n) - 10, n, overflowed=True)
  capacity, mapper, split, seg_len, run_ptr = rec.plan(False, *SPLIT_DEFAULTS)
  assert (mapper, split, seg_len) == (_lib.MAPPER_DIRECT, 0, 0) and capacity == rec.capacity > 0
  assert run_ptr == words[0].data_ptr() and len(words) == 1
  # many: the pre-sort, still without segments
  rec.observe(int(frame.PRESORT_ABOVE * n) + 10, n, overflowed=False)
  assert rec.plan(False, *SPLIT_DEFAULTS)[1:3] == (_lib.MAPPER_PRESORT, 0)
  # the split switches: off beats everything, always carries the segments on any frame, the threshold travels
  assert rec.plan(False, True, True, 0, 0)[2:4] == (1, 0)
  assert rec.plan(False, True, True, 512, 256)[2:4] == (512, 256)
  assert rec.plan(False, True, True, 1, 0)[2] == 2
  assert rec.plan(False, False, True, 512, 256)[2:4] == (0, 256)
  assert frame.ShapeRecord().plan(False, False, False, 0, 0)[1:3] == (_lib.MAPPER_PRESORT, 0)


def test_a_long_run_makes_the_shape_sticky_presort_with_segments_whatever_its_overlaps(words):
  rec = frame.ShapeRecord()
  n = 1000
  rec.plan(False, *SPLIT_DEFAULTS)
  rec.observe(2 * n, n, overflowed=True)
  assert rec.plan(False, *SPLIT_DEFAULTS)[1:3] == (_lib.MAPPER_DIRECT, 0) and not rec.sticky
  words[0][0] = frame.LONG_RUN_LIMIT                       # at the limit: not yet
  assert rec.plan(False, *SPLIT_DEFAULTS)[1:3] == (_lib.MAPPER_DIRECT, 0) and not rec.sticky
  words[0][0] = frame.LONG_RUN_LIMIT + 1
  assert rec.plan(False, *SPLIT_DEFAULTS)[1:3] == (_lib.MAPPER_PRESORT, 1) and rec.sticky
  words[0][0] = 0                                          # the pre-sort reports no run: the shape stays where it is
  rec.observe(n // 2, n, overflowed=False)
  assert rec.mapper == _lib.MAPPER_PRESORT
  assert rec.plan(False, *SPLIT_DEFAULTS)[1:3] == (_lib.MAPPER_PRESORT, 1) and rec.sticky
  assert rec.plan(False, False, False, 0, 0)[1:3] == (_lib.MAPPER_PRESORT, 0)      # MS_SPLIT_LONG_RUNS=0
  # a captured frame reads the word of the eager frames before it
  assert rec.plan(True, *SPLIT_DEFAULTS)[4] == words[0].data_ptr() and len(words) == 1


def test_depth16_shapes_always_take_the_presort(words):
  cfg = RasterConfig()
  key = frame._shape_key(torch.device('cuda', 0), 1000, (64, 64), cfg, None, True)
  plain = frame._shape_key(torch.device('cuda', 0), 1000, (64, 64), cfg, None, False)
  try:
    rec = frame.shape_record(key, create=True)
    assert rec.depth16 and not frame.shape_record(plain, create=True).depth16
    assert frame.shape_record(('2d',) + key, create=True).depth16
    for k_total in (10, 2000, 5000, 10):
      rec.observe(k_total, 1000, overflowed=False)
      assert rec.mapper == _lib.MAPPER_PRESORT
      assert rec.plan(False, *SPLIT_DEFAULTS)[1:3] == (_lib.MAPPER_PRESORT, 0)
  finally:
    for k in (key, plain, ('2d',) + key):
      frame._shapes.pop(k, None)


def test_capacity_is_granular_capped_and_never_shrinks():
  rec = frame.ShapeRecord()
  seen = []
  for k_total in (1, 100_000, 50_000, 3_000_000, 10, (1 << 31) - 1, 7):
    rec.observe(k_total, 1000, overflowed=False)
    want = min(-(-int(k_total * frame.K_SLACK) // frame.K_GRANULE) * frame.K_GRANULE, (1 << 31) - 1)
    assert rec.capacity >= want and (rec.capacity % frame.K_GRANULE == 0 or rec.capacity == (1 << 31) - 1)
    assert not seen or rec.capacity >= seen[-1]
    seen.append(rec.capacity)
  assert seen[0] == frame.K_GRANULE and seen[1] == seen[2] == 2 * frame.K_GRANULE and seen[-1] == (1 << 31) - 1
  assert frame.round_capacity(0) == frame.K_GRANULE and frame.round_capacity(frame.K_GRANULE + 1) == 2 * frame.K_GRANULE
  assert frame.round_capacity(1 << 40) == (1 << 31) - 1


def test_stable_count_resets_on_overflow_and_lazy_settle_flips_at_lazy_after():
  key = ('lazy-shape',)
  default = frame.LAZY_SETTLE
  try:
    frame.LAZY_SETTLE = True
    rec = frame.shape_record(key, create=True)
    rec.observe(5000, 1000, overflowed=True)               # the first frame of a shape always overflows (capacity 0)
    assert rec.stable == 0
    for i in range(1, frame.LAZY_AFTER + 1):
      assert not frame.lazy_settle_allowed(key)
      rec.observe(5000, 1000, overflowed=False)
      assert rec.stable == i
    assert frame.lazy_settle_allowed(key) == (not frame.STRICT)
    rec.observe(500_000, 1000, overflowed=True)
    assert rec.stable == 0 and not frame.lazy_settle_allowed(key)
  finally:
    frame.LAZY_SETTLE = default
    frame._shapes.pop(key, None)


def test_release_keeps_and_zeroes_the_run_word_unless_forced(words):
  key, bare = ('released-shape',), ('bare-shape',)
  try:
    rec = frame.shape_record(key, create=True)
    rec.plan(False, *SPLIT_DEFAULTS)
    words[0][0] = frame.LONG_RUN_LIMIT + 5
    rec.plan(False, *SPLIT_DEFAULTS)
    rec.observe(5000, 1000, overflowed=False)
    frame.shape_record(bare, create=True).capacity = 1 << 16       # (as set_overlap_capacity leaves one: no run word)
    frame._release_caches()
    # a frame in flight or a captured graph still writes the word: same storage, zero, and the shape starts over
    assert frame.shape_record(key) is rec and frame.shape_record(bare) is None
    assert rec.run_word is words[0] and int(words[0][0]) == 0
    assert (rec.capacity, rec.mapper, rec.sticky, rec.stable) == (0, None, False, 0)
    assert rec.plan(False, *SPLIT_DEFAULTS) == (0, _lib.MAPPER_PRESORT, 1, 0, words[0].data_ptr()) and len(words) == 1
    frame._release_caches(force=True)
    assert frame.shape_record(key) is None and rec.run_word is None and rec.run_view is None
  finally:
    frame._shapes.pop(key, None)
    frame._shapes.pop(bare, None)


def test_a_plan_under_capture_allocates_nothing(words):
  rec = frame.ShapeRecord()
  rec.capacity = 1 << 16
  capacity, mapper, split, seg_len, run_ptr = rec.plan(True, *SPLIT_DEFAULTS)
  assert (capacity, mapper, split, run_ptr) == (1 << 16, _lib.MAPPER_PRESORT, 1, None)
  assert words == [] and rec.run_word is None and rec.run_view is None
  assert frame.shape_record(('never-made',)) is None


def test_mapper_choice_follows_overlaps_per_gaussian_with_hysteresis():
  # frame.py picks the mapper's launch sequence per scene shape from the last overlap total (same lists either way):
  # depth pre-sort above ~3.5 overlaps per gaussian, storage-order emission + per-tile depth sort below
  key = ('test-shape',)
  try:
    n = 1000
    rec = frame.shape_record(key, create=True)
    rec.choose_mapper(2100, n)
    assert frame.shape_record(key).mapper == _lib.MAPPER_DIRECT
    rec.choose_mapper(int(frame.PRESORT_ABOVE * n) + 10, n)
    assert frame.shape_record(key).mapper == _lib.MAPPER_PRESORT
    rec.choose_mapper(int(0.5 * (frame.PRESORT_ABOVE + frame.DIRECT_BELOW) * n), n)                   # inside the band: stays
    assert frame.shape_record(key).mapper == _lib.MAPPER_PRESORT
    rec.choose_mapper(int(frame.DIRECT_BELOW * n) - 10, n)
    assert frame.shape_record(key).mapper == _lib.MAPPER_DIRECT
    rec.choose_mapper(int(0.5 * (frame.PRESORT_ABOVE + frame.DIRECT_BELOW) * n), n)
    assert frame.shape_record(key).mapper == _lib.MAPPER_DIRECT
  finally:
    frame._shapes.pop(key, None)


def test_split_policy_and_lazy_settle_switches():
  try:
    frame.set_split_policy(min_run=512, seg_len=256, always=True)
    assert (frame.SPLIT_MIN_RUN, frame.SPLIT_SEG_LEN, frame.SPLIT_ALWAYS) == (512, 256, True)
    with pytest.raises(AssertionError):
      frame.set_split_policy(min_run=-1)
  finally:
    frame.set_split_policy()
  assert (frame.SPLIT_MIN_RUN, frame.SPLIT_SEG_LEN, frame.SPLIT_ALWAYS) == (0, 0, False)
  # lazy settle: opt-in, and only for shapes whose capacity has been stable for LAZY_AFTER settled frames
  key = ('shape',)
  default = frame.LAZY_SETTLE
  try:
    frame.LAZY_SETTLE = False
    frame.shape_record(key, create=True).stable = 10
    assert not frame.lazy_settle_allowed(key)
    frame.LAZY_SETTLE = True
    assert frame.lazy_settle_allowed(key) == (not frame.STRICT)
    frame.shape_record(key).stable = frame.LAZY_AFTER - 1
    assert not frame.lazy_settle_allowed(key)
    assert not frame.lazy_settle_allowed(('unknown',))
  finally:
    frame.LAZY_SETTLE = default
    frame._shapes.pop(key, None)
  frame.settle_all()                       # nothing queued: returns at once


def test_frame_state_settles_once_and_only_lazy_frames_skip_the_wait():
  calls = []
  st = frame.FrameState()
  st.pending = lambda at_entry=False: calls.append(at_entry)
  st.settle(); st.settle()
  assert calls == [False] and st.pending is None
  # backward of a frame that was NOT queued lazily waits (round 5's behaviour for callers of the bare Function)
  st = frame.FrameState()
  st.pending = lambda at_entry=False: calls.append('waited')
  st.k_peek = np.array([frame.K_PENDING], dtype=np.int32)
  assert st.settle_if_known() and calls[-1] == 'waited' and not st.consumed
  # a lazily queued frame whose total is not there yet: the backward goes ahead and the frame is marked
  st = frame.FrameState()
  st.lazy = True
  st.pending = lambda at_entry=False: calls.append('never')
  st.k_peek = np.array([frame.K_PENDING], dtype=np.int32)
  assert st.settle_if_known() is False and st.consumed and calls[-1] != 'never'
  st.k_peek[0] = 1234                       # ... and once it is there, settling costs no wait
  assert st.settle_if_known() and calls[-1] == 'never'


def test_deferred_visibility_bookkeeping_without_a_device():
  """frame.VISIBILITY_FROM_BACKWARD is opt-in; a frame state that is not deferred, or whose backward pass has written the
  sums, never runs the pass on demand (no library call is made here: the early returns)."""
  assert frame.VISIBILITY_FROM_BACKWARD is False and frame.SH_SIDE_STREAM is True
  st = frame.FrameState()
  assert (st.vis_deferred, st.vis_ready, st.vis_pass, st.colours_ready) == (False, True, None, None)
  passes = frame.visibility_passes
  st.ensure_visibility()                                       # not deferred
  st.vis_deferred, st.vis_ready = True, True
  st.ensure_visibility()                                       # deferred and already written by the backward pass
  assert frame.visibility_passes == passes
  # the grads struct carries the pointer the per-gaussian pass writes the sums through, and the header agrees on its place
  # (tests/test_abi.py holds every offset against a C compiler)
  gr = _lib.FrameGradsC()
  assert gr.point_visibility is None and gr.struct_size == ctypes.sizeof(_lib.FrameGradsC)
  names = [f[0] for f in _lib.FrameGradsC._fields_]
  assert names.index('point_visibility') == names.index('point_heuristic') + 1
  assert 'ms_frame_sh_colours' in _lib.SIGNATURES


def test_identity_indexes_made_under_inference_mode_serve_training_frames():
  frame._identity.clear()
  dev = torch.device('cpu')
  with torch.inference_mode():
    idx = frame.identity_indexes(7, dev)
  assert not idx.is_inference()
  feature = torch.rand(7, 3, requires_grad=True)
  feature[frame.identity_indexes(7, dev)].sum().backward()       # "Inference tensors cannot be saved for backward"
  assert feature.grad is not None
  assert frame.identity_indexes(7, dev) is idx


def test_frame_layout_query_and_dispatch_without_a_gpu():
  lib = _lib.load()
  cfg = RasterConfig()
  d = _lib.FrameDescC(n=1000, k_capacity=5000, image_w=250, image_h=130, dtype=_lib.MS_F32, f=3, sh_degree=3, depth16=0,
                      tile_row_begin=0, tile_row_end=1 << 30, projected_input=0, raster=_lib.raster_config_c(cfg))
  lay = _lib.FrameLayoutC()
  assert lib.ms_frame_layout_query(ctypes.byref(d), ctypes.byref(lay)) == 0
  tiles = ((250 + 15) // 16) * ((130 + 15) // 16)
  assert lay.keep_n_bytes >= 1000 * (28 + 4 + 12) + tiles * 8 and lay.keep_k_bytes >= 5000 * 4
  offsets = [lay.points7, lay.depth, lay.colours, lay.camera_position, lay.counters, lay.tile_ranges]
  assert offsets == sorted(offsets) and all(o % 256 == 0 for o in offsets)
  assert lib.ms_frame_uses_moments(ctypes.byref(d), 0) == 1
  d.raster.tile_size = 32                # the scan backward serves every tile size since the 1024-thread tile-32 variant
  assert lib.ms_frame_uses_moments(ctypes.byref(d), 0) == 1 and lib.ms_frame_uses_moments(ctypes.byref(d), 1) == 1
  d.raster.tile_size = 16; d.raster.antialias = 1
  assert lib.ms_frame_uses_moments(ctypes.byref(d), 0) == 0
  d.f = 7                        # no instantiation: argument error, not a crash
  assert lib.ms_frame_layout_query(ctypes.byref(d), ctypes.byref(lay)) == -2
  d.f = 3; d.projected_input = 1  # projected input cannot carry SH
  assert lib.ms_frame_layout_query(ctypes.byref(d), ctypes.byref(lay)) == -1


def test_parked_gc_restores_the_collector():
  """frame.parked_gc: the collector is off inside the block and back to its previous state after it, also on error"""
  assert gc.isenabled()
  with frame.parked_gc():
    assert not gc.isenabled()
  assert gc.isenabled()
  try:
    with frame.parked_gc():
      raise ValueError("boom")
  except ValueError:
    pass
  assert gc.isenabled()
  gc.disable()
  try:
    with frame.parked_gc():
      pass
    assert not gc.isenabled()            # it was off before: stays off
  finally:
    gc.enable()
