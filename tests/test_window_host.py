"""CPU tests of the host side between tensors and the ``ms_frame_*`` / ``ms_raster_*`` structs: the row window of a render
(``_window.RowWindow``: clamped tile rows, pixel rows, stored shape, zero-fill rule, kernel base address, the window that
stores no row), dL/dimage as an expanded scalar (``frame.image_grad``) and the per-gaussian inputs and gradients
(``frame.gaussian_inputs`` / ``gaussian_grads``).  No kernel runs; CPU tensors only."""
import itertools

import pytest
import torch

from taichi_splatting_amd import RasterConfig, _lib, frame
from taichi_splatting_amd._window import RowWindow

W = 5
HEIGHTS, TILE_SIZES = (16, 17, 33, 97), (8, 16, 32)
DEV = torch.device('cpu')


def tile_row_cases(tiles_high):
  return (None, (0, 1), (1, 3), (tiles_high - 1, tiles_high), (tiles_high, tiles_high), (2, 2), (-1, 99), (0, tiles_high))


def all_windows():
  for h, ts, cropped in itertools.product(HEIGHTS, TILE_SIZES, (False, True)):
    tiles_high = -(-h // ts)
    for tile_rows in tile_row_cases(tiles_high):
      yield h, ts, tiles_high, tile_rows, cropped, RowWindow.of((W, h), ts, tile_rows, cropped)


def test_rows_pixels_whole_and_stored_shape_follow_the_closed_form():
  for h, ts, tiles_high, tile_rows, cropped, win in all_windows():
    case = (h, ts, tile_rows, cropped)
    # frame_geom (csrc/frame.hip): begin below 0 becomes 0, end above tiles_high becomes tiles_high, nothing else moves
    b, e = (0, tiles_high) if tile_rows is None else tile_rows
    b, e = (0 if b < 0 else b), (tiles_high if e > tiles_high else e)
    assert win.rows == (b, e) and (win.w, win.h, win.cropped) == (W, h, cropped), case
    assert win.px_rows == (win.y0, win.y1) == (min(b * ts, h), min(e * ts, h)), case
    assert win.whole == (b == 0 and e == tiles_high), case
    assert win.stored_rows == (win.y1 - win.y0 if cropped else h), case
    assert win.alloc(torch.float32, DEV, 3).shape == (win.stored_rows, W, 3), case
    assert win.alloc(torch.float64, DEV).shape == (win.stored_rows, W), case
    with pytest.raises(AttributeError):
      win.y0 = 0                                       # a value: nobody edits a window
  # frame_desc hands the same rows to the C side
  desc, rows = frame.frame_desc(10, (W, 33), torch.float32, 3, -1, RasterConfig(tile_size=16), tile_rows=(-1, 99))
  assert rows == (0, 3) == (desc.tile_row_begin, desc.tile_row_end) and (desc.image_w, desc.image_h) == (W, 33)
  assert frame.frame_desc(10, (W, 33), torch.float32, 3, -1, RasterConfig(tile_size=16), tile_rows=(2, 2))[1] == (2, 2)


def test_only_a_window_neither_cropped_nor_whole_is_zeroed(monkeypatch):
  # torch.empty recycles memory: stand in an allocator whose "uninitialised" memory is visibly so
  poisoned = lambda shape, dtype, device: torch.full(shape, 7.0, dtype=dtype, device=device)
  monkeypatch.setattr(torch, 'empty', poisoned)
  seen = set()
  for h, ts, tiles_high, tile_rows, cropped, win in all_windows():
    want_zero = not cropped and not win.whole
    assert win.zero_filled == want_zero
    for t in (win.alloc(torch.float32, DEV, 3), win.alloc(torch.float32, DEV)):
      assert bool((t == 0).all()) == want_zero or t.numel() == 0, (h, ts, tile_rows, cropped)
    scratch = win.alloc(torch.float32, DEV, 3, scratch=True)              # never filled, whatever the window
    assert scratch.numel() == 0 or bool((scratch == 7.0).all())
    seen.add((want_zero, win.stored_rows == 0))
  assert seen == {(True, False), (False, False), (False, True)}


def test_base_address_is_where_row_zero_would_be():
  for h, ts, tiles_high, tile_rows, cropped, win in all_windows():
    if win.stored_rows == 0:
      continue                                          # (the next test)
    assert win.placeholder(torch.float32, DEV) is None              # nothing is allocated for a window that stores rows
    first = win.y0 if cropped else 0
    for c, dtype in itertools.product((1, 3), (torch.float32, torch.float64)):
      t = win.alloc(dtype, DEV, c)
      assert win.base(t, c) + first * W * c * t.element_size() == t.data_ptr(), (h, ts, tile_rows, cropped, c, dtype)
    flat = win.alloc(torch.float32, DEV)
    assert win.base(flat) + first * W * 4 == flat.data_ptr()
    with pytest.raises(AssertionError):
      win.base(torch.zeros(win.stored_rows + 1, W, 3), 3)           # a tensor laid out for another window


def test_a_window_that_stores_no_row_hands_out_its_placeholder_and_nothing_else():
  empty = [(h, ts, tile_rows, win) for h, ts, _, tile_rows, cropped, win in all_windows() if win.stored_rows == 0]
  assert len(empty) == 27 and all(win.cropped for *_, win in empty)
  for h, ts, tile_rows, win in empty:
    assert win.y1 <= win.y0
    hold = win.placeholder(torch.float32, DEV)
    lo, hi = hold.data_ptr(), hold.data_ptr() + hold.numel() * hold.element_size()
    for c in (1, 3):
      t = win.alloc(torch.float32, DEV, c)
      assert t.shape[0] == 0
      assert lo <= win.base(t, c, hold) < hi, (h, ts, tile_rows)
    with pytest.raises(AssertionError):
      win.base(win.alloc(torch.float32, DEV, 3), 3)     # no placeholder: an error, never an address made from a null pointer
  # the bottom of an image whose height is no tile multiple: both ends are clamped to h
  assert RowWindow.of((W, 17), 8, (3, 3)).px_rows == (17, 17)


class TestImageGrad:
  window = RowWindow.of((5, 150), 16, (3, 9), cropped=True)               # pixel rows [48, 144)

  def run(self, g, moments_path=True):
    gr = _lib.FrameGradsC()
    keep = frame.image_grad(gr, g, moments_path, self.window, 3)
    return gr, keep

  def test_an_expanded_scalar_is_handed_over_as_one_pixel(self):
    assert frame.BROADCAST_GRAD is True
    image = torch.zeros(96, 5, 3, requires_grad=True)
    (from_sum,) = torch.autograd.grad(image.sum(), image)
    assert from_sum.stride() == (0, 0, 0)
    for g in (torch.tensor(1.).expand(7, 5, 3), from_sum):
      gr, keep = self.run(g)
      assert gr.grad_image_broadcast == 1 and keep.shape == (3,) and keep.is_contiguous()
      assert gr.grad_image == keep.data_ptr()                             # not offset by the window
      assert torch.equal(keep, torch.ones(3))

  def test_everything_else_is_dense_and_offset_by_the_window(self, monkeypatch):
    dense = torch.rand(96, 5, 3)
    rows_only = torch.rand(1, 5, 3).expand(96, 5, 3)                      # stride(0) == 0, stride(1) != 0
    scalar = torch.tensor(1.).expand(96, 5, 3)
    cases = [(dense, True), (rows_only, True), (scalar, False)]
    for g, moments_path in cases:
      gr, keep = self.run(g, moments_path)
      assert gr.grad_image_broadcast == 0 and keep.is_contiguous() and torch.equal(keep, g)
      assert gr.grad_image + 48 * 5 * 3 * 4 == keep.data_ptr()
    assert self.run(dense)[1] is dense                                    # no copy of what is contiguous already
    monkeypatch.setattr(frame, 'BROADCAST_GRAD', False)                   # read at call time
    gr, keep = self.run(scalar)
    assert gr.grad_image_broadcast == 0 and keep.shape == (96, 5, 3) and gr.grad_image + 48 * 5 * 3 * 4 == keep.data_ptr()

  def test_one_pixel_is_dense(self):
    window = RowWindow.of((1, 1), 16)
    gr = _lib.FrameGradsC()
    keep = frame.image_grad(gr, torch.tensor(1.).expand(1, 1, 3), True, window, 3)
    assert gr.grad_image_broadcast == 0 and keep.shape == (1, 1, 3) and gr.grad_image == keep.data_ptr()

  def test_an_empty_strip_gets_the_placeholder(self):
    window = RowWindow.of((5, 150), 16, (3, 3), cropped=True)
    image = torch.zeros(0, 5, 3, requires_grad=True)
    (g,) = torch.autograd.grad(image.sum(), image)
    hold = window.placeholder(torch.float32, DEV)
    gr = _lib.FrameGradsC()
    frame.image_grad(gr, g, True, window, 3, hold)
    assert gr.grad_image_broadcast == 0 and gr.grad_image == hold.data_ptr()


def _gaussian_tensors(n, feature):
  return (torch.rand(n, 3), torch.rand(n, 3), torch.rand(n, 4), torch.rand(n, 1), feature, torch.eye(4), torch.rand(4))


def test_gaussian_inputs_parse_the_feature_tensor_and_point_at_contiguous_copies():
  n = 6
  args = _gaussian_tensors(n, torch.rand(n, 16, 3).transpose(1, 2).requires_grad_(True))        # (n, 3, 16), not contiguous
  tensors, inputs, f, degree = frame.gaussian_inputs(*args, True)
  assert (f, degree) == (3, 3) and len(tensors) == 7
  assert all(t.is_contiguous() and not t.requires_grad and torch.equal(t, a) for t, a in zip(tensors, args))
  names = ('position', 'log_scaling', 'rotation', 'alpha_logit', 'feature', 'T_camera_world', 'projection')
  assert [getattr(inputs, k) for k in names] == [t.data_ptr() for t in tensors]
  assert (inputs.points7, inputs.depth, inputs.colours) == (None, None, None)
  assert frame.gaussian_inputs(*_gaussian_tensors(n, torch.rand(n, 3)), False)[2:] == (3, -1)
  assert frame.gaussian_inputs(*_gaussian_tensors(n, torch.rand(n, 2, 1)), True)[2:] == (2, 0)
  with pytest.raises(AssertionError, match=r"SH feature count must be square, got 5 \(torch.Size\(\[6, 3, 5\]\)\)"):
    frame.gaussian_inputs(*_gaussian_tensors(n, torch.rand(n, 3, 5)), True)
  with pytest.raises(AssertionError, match=r"SH features must have 3 dimensions, got torch.Size\(\[6, 3\]\)"):
    frame.gaussian_inputs(*_gaussian_tensors(n, torch.rand(n, 3)), True)
  with pytest.raises(AssertionError, match="SH degree must be between 0 and 3, got 4"):
    frame.gaussian_inputs(*_gaussian_tensors(n, torch.rand(n, 3, 25)), True)
  with pytest.raises(AssertionError, match=r"Features must be \(N, C\) if use_sh=False"):
    frame.gaussian_inputs(*_gaussian_tensors(n, torch.rand(n, 3, 16)), False)


def test_gaussian_grads_allocate_what_is_needed_and_the_feature_gradient_only_when_the_kernel_writes_it():
  tensors = _gaussian_tensors(4, torch.rand(4, 3, 16))[:5]
  gr = _lib.FrameGradsC()
  grads, grad_feature = frame.gaussian_grads(gr, tensors, (True, False, True, True, True), True)
  assert [g is not None for g in grads] == [True, False, True, True]
  assert all(g is None or (g.shape == t.shape and g.dtype == t.dtype) for g, t in zip(grads, tensors))
  assert (gr.grad_position, gr.grad_log_scaling, gr.grad_rotation, gr.grad_alpha_logit) == \
    (grads[0].data_ptr(), None, grads[2].data_ptr(), grads[3].data_ptr())
  assert grad_feature.shape == (4, 3, 16) and gr.grad_feature == grad_feature.data_ptr()
  for need_feature, from_kernel in ((True, False), (False, True)):
    gr = _lib.FrameGradsC()
    grads, grad_feature = frame.gaussian_grads(gr, tensors, (False, True, False, False, need_feature), from_kernel)
    assert grad_feature is None and gr.grad_feature is None and gr.grad_log_scaling == grads[1].data_ptr()
    assert grads[0] is None and gr.grad_position is None
