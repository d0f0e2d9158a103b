"""The wide-feature rasteriser without a GPU: return codes of ms_raster_wide_fwd / ms_raster_wide_bwd and their
precedence (in the manner of tests/test_raster_args_host.py: every call returns before any launch, the pointers are
dummies), the Python errors of rasterize_wide / render_features, and the exports.

Precedence: every MS_ERR_BAD_ARG condition (null pointer, size, feature count, both gradients NULL — in that order) is
reported before any MS_ERR_UNSUPPORTED condition (tile size, antialias, no alpha blending — in that order)."""
import ctypes
from dataclasses import replace

import pytest
import torch

import taichi_splatting_amd as tsa
from taichi_splatting_amd import RasterConfig, _lib
from taichi_splatting_amd.rasterizer import wide

P = 0x10000        # a valid-looking pointer, never dereferenced
BAD_ARG, UNSUPPORTED = -1, -2


def config(**kw):
  args = dict(tile_size=16, antialias=0, use_alpha_blending=1, compute_visibility=0, compute_point_heuristic=0, reserved=0,
              clamp_max_alpha=0.99, alpha_threshold=1 / 255., saturate_threshold=0.9999)
  args.update(kw)
  return _lib.RasterConfigC(**args)


def cfg_pointer(kw):
  cfg = kw.pop('cfg', {})
  return None if cfg is None else ctypes.byref(config(**cfg))


def fwd(ptr=P, **kw):
  g = lambda k, d: kw.pop(k, d)
  cfg = cfg_pointer(kw)
  a = [g('points7', ptr), g('features', ptr), g('ranges', ptr), g('o2p', ptr), g('w', 64), g('h', 64), g('f', 32), cfg,
       g('out_image', ptr), g('out_alpha', ptr), None]
  assert not kw, kw
  return 'ms_raster_wide_fwd', a


def bwd(ptr=P, **kw):
  g = lambda k, d: kw.pop(k, d)
  cfg = cfg_pointer(kw)
  a = [g('points7', ptr), g('features', ptr), g('ranges', ptr), g('o2p', ptr), g('image', ptr), g('grad_image', ptr),
       g('w', 64), g('h', 64), g('f', 32), cfg, g('grad_points7', ptr), g('grad_features', ptr), None]
  assert not kw, kw
  return 'ms_raster_wide_bwd', a


CASES = []
def case(call, rc, keyword=None):
  CASES.append(pytest.param(call[0], call[1], rc, keyword, id=f"{len(CASES):02d}-{call[0][3:]}-rc{rc}"))


for e in (fwd, bwd):
  # null pointers
  case(e(cfg=None), BAD_ARG, b'null')
  case(e(ptr=None), BAD_ARG, b'null')
  for name in ('points7', 'features', 'ranges', 'o2p'):
    case(e(**{name: None}), BAD_ARG, b'null')
  # sizes
  case(e(w=0), BAD_ARG, b'size')
  case(e(h=-3), BAD_ARG, b'size')
  # feature counts: 1..128
  case(e(f=0), BAD_ARG, b'feature size 0')
  case(e(f=-1), BAD_ARG, b'feature size -1')
  case(e(f=129), BAD_ARG, b'feature size 129')
  # unsupported configurations
  case(e(cfg=dict(tile_size=8)), UNSUPPORTED, b'tile_size')
  case(e(cfg=dict(tile_size=32)), UNSUPPORTED, b'tile_size')
  case(e(cfg=dict(antialias=1)), UNSUPPORTED, b'antialias')
  case(e(cfg=dict(use_alpha_blending=0)), UNSUPPORTED, b'use_alpha_blending')
  # precedence: -1 before -2, and within each class the documented order
  case(e(cfg=dict(tile_size=8), ptr=None), BAD_ARG, b'null')
  case(e(cfg=dict(tile_size=8), w=0), BAD_ARG, b'size')
  case(e(cfg=dict(antialias=1), f=200), BAD_ARG, b'feature size 200')
  case(e(w=0, f=200), BAD_ARG, b'size')
  case(e(ranges=None, w=0), BAD_ARG, b'null')
  case(e(cfg=dict(tile_size=8, antialias=1, use_alpha_blending=0)), UNSUPPORTED, b'tile_size')
  case(e(cfg=dict(antialias=1, use_alpha_blending=0)), UNSUPPORTED, b'antialias')
  # heuristics / visibility switches are ignored, not refused
  case(e(cfg=dict(compute_visibility=1, compute_point_heuristic=1, tile_size=8)), UNSUPPORTED, b'tile_size')
for name in ('out_image', 'out_alpha'):
  case(fwd(**{name: None}), BAD_ARG, b'null')
for name in ('image', 'grad_image'):
  case(bwd(**{name: None}), BAD_ARG, b'null')
case(bwd(grad_points7=None, grad_features=None), BAD_ARG, b'both null')
case(bwd(grad_points7=None, grad_features=None, f=0), BAD_ARG, b'feature size 0')            # the feature count comes first
case(bwd(grad_points7=None, grad_features=None, cfg=dict(tile_size=8)), BAD_ARG, b'both null')   # ... and -1 before -2
case(bwd(grad_points7=None, cfg=dict(antialias=1)), UNSUPPORTED, b'antialias')               # one gradient is enough
case(bwd(grad_features=None, cfg=dict(antialias=1)), UNSUPPORTED, b'antialias')


@pytest.mark.parametrize("name, args, rc, keyword", CASES)
def test_wide_entry_point_checks_its_arguments(lib, name, args, rc, keyword):
  got = getattr(lib, name)(*args)
  message = lib.ms_last_error_string()
  assert got == rc, (name, got, rc, message)
  if keyword is not None:
    assert keyword in message, (name, keyword, message)


def test_version_is_unchanged_and_limit_is_exported(lib):
  assert lib.ms_version() == 501
  assert wide.MAX_WIDE_FEATURES == 128
  header = (_lib.CSRC_DIR.parent.parent / 'include' / 'mi355_splat.h').read_text()
  assert '#define MS_RASTER_WIDE_MAX_F 128' in header


def test_exports():
  from taichi_splatting_amd import rasterizer
  for module in (tsa, rasterizer):
    assert module.rasterize_wide is wide.rasterize_wide
    assert module.render_features is wide.render_features
    assert 'rasterize_wide' in module.__all__ and 'render_features' in module.__all__
  assert set(('ms_raster_wide_fwd', 'ms_raster_wide_bwd')) <= set(_lib.SIGNATURES)


class FakeCuda(torch.Tensor):
  """a CPU tensor that says it is on the GPU: the argument checks run before anything touches a device"""
  @staticmethod
  def __new__(cls, t):
    return torch.Tensor._make_subclass(cls, t)
  is_cuda = True


def wide_args(n=4, f=8, dtype=torch.float32, size=(32, 16), cuda=True):
  wrap = FakeCuda if cuda else (lambda t: t)
  return (wrap(torch.zeros((n, 7), dtype=dtype)), wrap(torch.zeros((n, f), dtype=dtype)),
          wrap(torch.zeros((0,), dtype=torch.int32)), wrap(torch.zeros((2, 2), dtype=torch.int32)), size)


@pytest.mark.parametrize('args, cfg, error, keyword', [
  (wide_args(dtype=torch.float64), RasterConfig(tile_size=16), NotImplementedError, 'float32'),
  (wide_args(), RasterConfig(tile_size=8, pixel_stride=(1, 1)), NotImplementedError, 'tile_size 8'),
  (wide_args(), RasterConfig(tile_size=32), NotImplementedError, 'tile_size 32'),
  (wide_args(), RasterConfig(tile_size=16, antialias=True), NotImplementedError, 'antialias'),
  (wide_args(), RasterConfig(tile_size=16, use_alpha_blending=False), NotImplementedError, 'use_alpha_blending'),
  (wide_args(f=129), RasterConfig(tile_size=16), ValueError, '129 feature channels'),
  (wide_args(f=0), RasterConfig(tile_size=16), ValueError, '0 feature channels'),
  (wide_args(cuda=False), RasterConfig(tile_size=16), ValueError, 'GPU only'),
  (wide_args(size=(64, 64)), RasterConfig(tile_size=16), ValueError, 'needs 16'),
])
def test_rasterize_wide_refuses_what_it_does_not_serve(args, cfg, error, keyword):
  with pytest.raises(error, match=keyword):
    tsa.rasterize_wide(*args, cfg)


def test_render_features_needs_a_frame_rendering():
  class NotAFrame:
    pass
  with pytest.raises(ValueError, match='rasterize_wide'):
    tsa.render_features(NotAFrame(), torch.zeros((4, 8)))

  from taichi_splatting_amd._window import RowWindow

  class Strip:
    class frame:
      window = RowWindow.of((64, 64), 16, tile_rows=(1, 3))
    frame_points7 = torch.zeros((4, 7))
  with pytest.raises(NotImplementedError, match='tile_rows'):
    tsa.render_features(Strip(), torch.zeros((4, 8)))
