"""Argument checks of the nine raster entry points of the C-ABI: return codes, their precedence and a keyword of the
error message.  Every call below returns before any launch (the checks come first, as in
test_abi.py::test_split_parameters_size_the_scratch), so the pointers are dummies and no device is needed.

The table is the recorded behaviour of the library before the raster host got its one argument record: null checks
come AFTER the configuration checks on ms_raster_fwd / ms_raster_bwd and BEFORE them on the three
ms_raster_bwd_moments* entry points; ms_raster_fwd_rows / _split look at their own pointers (cfg, rows, scratch) first
and at the shared ones after the configuration."""
import ctypes

import pytest

from taichi_splatting_amd import _lib

P = 0x10000        # a valid-looking pointer: 256-byte aligned, never dereferenced
ODD = P + 16       # neither 64- nor 256-byte aligned
BAD_ARG, UNSUPPORTED = -1, -2


def config(**kw):
  args = dict(tile_size=16, antialias=0, use_alpha_blending=1, compute_visibility=0, compute_point_heuristic=0, reserved=0,
              clamp_max_alpha=0.99, alpha_threshold=1 / 255., saturate_threshold=0.9999)
  args.update(kw)
  return _lib.RasterConfigC(**args)


def cfg_pointer(kw):
  cfg = kw.pop('cfg', {})
  return None if cfg is None else ctypes.byref(config(**cfg))


# One builder per entry point: keyword arguments -> the positional list of include/mi355_splat.h.  `ptr` is the default
# of every pointer that is not named (P: valid-looking, None: null); the window defaults to tile rows [0, 4).
def fwd(ptr=P, **kw):
  g = lambda k, d: kw.pop(k, d)
  cfg = cfg_pointer(kw)
  a = [g('points7', ptr), g('features', ptr), g('ranges', ptr), g('o2p', ptr), g('w', 64), g('h', 64), g('f', 3), cfg,
       g('out_image', ptr), g('out_alpha', ptr), g('out_visibility', None), g('row_begin', 0), g('row_end', 4),
       g('dtype', _lib.MS_F32), None]
  assert not kw, kw
  return 'ms_raster_fwd', a


def fwd_split(ptr=P, **kw):
  g = lambda k, d: kw.pop(k, d)
  cfg = cfg_pointer(kw)
  a = [g('points7', ptr), g('features', ptr), g('ranges', ptr), g('o2p', ptr), g('k_capacity', 100), g('w', 64), g('h', 64),
       cfg, g('out_image', ptr), g('out_alpha', ptr), g('out_visibility', None), g('scratch', ptr), g('min_run', 0),
       g('seg_len', 0), g('row_begin', 0), g('row_end', 4), None]
  assert not kw, kw
  return 'ms_raster_fwd_split', a


def fwd_rows(ptr=P, **kw):
  g = lambda k, d: kw.pop(k, d)
  cfg = cfg_pointer(kw)
  a = [g('rows', ptr), g('ranges', ptr), g('o2p', ptr), g('w', 64), g('h', 64), cfg, g('out_image', ptr), g('out_alpha', ptr),
       g('out_visibility', None), g('row_begin', 0), g('row_end', 4), None]
  assert not kw, kw
  return 'ms_raster_fwd_rows', a


def bwd(ptr=P, **kw):
  g = lambda k, d: kw.pop(k, d)
  cfg = cfg_pointer(kw)
  a = [g('points7', ptr), g('features', ptr), g('ranges', ptr), g('o2p', ptr), g('image', ptr), g('grad_image', ptr),
       g('w', 64), g('h', 64), g('f', 3), cfg, g('grad_points7', ptr), g('grad_features', ptr), g('point_heuristic', None),
       g('row_begin', 0), g('row_end', 4), g('dtype', _lib.MS_F32), None]
  assert not kw, kw
  return 'ms_raster_bwd', a


def moments(ptr=P, **kw):
  g = lambda k, d: kw.pop(k, d)
  cfg = cfg_pointer(kw)
  a = [g('points7', ptr), g('features', ptr), g('ranges', ptr), g('o2p', ptr), g('image', ptr), g('grad_image', ptr),
       g('w', 64), g('h', 64), cfg, g('moments', ptr), g('deterministic', 0), g('fixed_exp', None), g('row_begin', 0),
       g('row_end', 4), None]
  assert not kw, kw
  return 'ms_raster_bwd_moments', a


def moments_rows(ptr=P, **kw):
  g = lambda k, d: kw.pop(k, d)
  cfg = cfg_pointer(kw)
  a = [g('rows', ptr), g('ranges', ptr), g('o2p', ptr), g('image', ptr), g('grad_image', ptr), g('w', 64), g('h', 64), cfg,
       g('moments', ptr), g('deterministic', 0), g('fixed_exp', None), g('row_begin', 0), g('row_end', 4), None]
  assert not kw, kw
  return 'ms_raster_bwd_moments_rows', a


def moments_split(ptr=P, **kw):
  g = lambda k, d: kw.pop(k, d)
  cfg = cfg_pointer(kw)
  a = [g('points7', ptr), g('features', ptr), g('ranges', ptr), g('o2p', ptr), g('k_capacity', 100), g('image', ptr),
       g('grad_image', ptr), g('w', 64), g('h', 64), cfg, g('moments', ptr), g('deterministic', 0), g('fixed_exp', None),
       g('scratch', ptr), g('min_run', 0), g('seg_len', 0), g('row_begin', 0), g('row_end', 4), None]
  assert not kw, kw
  return 'ms_raster_bwd_moments_split', a


def finalize(ptr=P, **kw):
  g = lambda k, d: kw.pop(k, d)
  a = [g('points7', ptr), g('moments', ptr), g('deterministic', 0), g('fixed_exp', None), g('n', 10), g('grad_points7', ptr),
       g('grad_features', ptr), g('point_heuristic', None), None]
  assert not kw, kw
  return 'ms_raster_moments_finalize', a


def pack(ptr=P, **kw):
  g = lambda k, d: kw.pop(k, d)
  a = [g('points7', ptr), g('depth', None), g('colours', ptr), g('n', 10), g('rows', ptr), None]
  assert not kw, kw
  return 'ms_splat_rows_pack', a


WINDOWED = (fwd, fwd_split, fwd_rows, bwd, moments, moments_rows, moments_split)
CONFIGURED = WINDOWED
EMPTY = dict(row_begin=2, row_end=2)
HEUR = dict(compute_point_heuristic=1)

CASES = []
def case(call, rc, keyword=None):
  CASES.append(pytest.param(call[0], call[1], rc, keyword, id=f"{len(CASES):02d}-{call[0][3:]}-rc{rc}"))


# ---- null cfg: -1 everywhere
for e in CONFIGURED:
  case(e(cfg=None), BAD_ARG, b'null')
  case(e(cfg=None, ptr=None), BAD_ARG, b'null')

# ---- bad image size: -1 (the moments entry points take no dtype)
for e in CONFIGURED:
  case(e(w=0), BAD_ARG, b'size')
  case(e(w=64, h=-3), BAD_ARG, b'size')
for e in (fwd, bwd):
  case(e(dtype=7), BAD_ARG, b'dtype')
  case(e(dtype=7, ptr=None), BAD_ARG, b'dtype')        # ... and before the null checks

# ---- tile size 12: -2; before the null checks on ms_raster_fwd / ms_raster_bwd (test_abi.py relies on it) ...
for e in (fwd, bwd):
  case(e(cfg=dict(tile_size=12), ptr=None), UNSUPPORTED, b'tile_size')
  case(e(cfg=dict(tile_size=12)), UNSUPPORTED, b'tile_size')
  case(e(cfg=dict(tile_size=12), f=5), UNSUPPORTED, b'tile_size')     # the tile size is looked at before the feature count
  case(e(cfg=dict(tile_size=12), dtype=7), BAD_ARG, b'dtype')         # ... and after the dtype
# ... after them on the moments entry points ...
for e in (moments, moments_rows, moments_split):
  case(e(cfg=dict(tile_size=12), ptr=None), BAD_ARG, b'null')
  case(e(cfg=dict(tile_size=12)), UNSUPPORTED, b'tile_size')
# ... and the rows / split forwards check the pointers only they have first, the shared ones after the configuration
case(fwd_rows(cfg=dict(tile_size=12), ptr=None), BAD_ARG, b'null')
case(fwd_rows(cfg=dict(tile_size=12), ptr=None, rows=P), UNSUPPORTED, b'tile')
case(fwd_rows(cfg=dict(tile_size=12)), UNSUPPORTED, b'tile')
case(fwd_split(cfg=dict(tile_size=12), ptr=None), BAD_ARG, b'null')
case(fwd_split(cfg=dict(tile_size=12), ptr=None, scratch=P), UNSUPPORTED)
case(fwd_split(cfg=dict(tile_size=12)), UNSUPPORTED)

# ---- null pointers with a good configuration: -1
for e in WINDOWED:
  case(e(ranges=None), BAD_ARG, b'null')
for e in (fwd, fwd_split, fwd_rows):
  case(e(out_image=None), BAD_ARG, b'null')
  case(e(out_alpha=None), BAD_ARG, b'null')
for e in (bwd, moments, moments_rows, moments_split):
  case(e(image=None), BAD_ARG, b'null')
  case(e(grad_image=None), BAD_ARG, b'null')
for e in (moments, moments_rows, moments_split):
  case(e(moments=None), BAD_ARG, b'null')
case(fwd_rows(rows=None), BAD_ARG, b'null')
case(moments_rows(rows=None), BAD_ARG, b'null')
case(moments(points7=None), BAD_ARG, b'null')
case(moments(features=None), BAD_ARG, b'null')

# ---- ms_raster_fwd / ms_raster_bwd: feature counts
for e in (fwd, bwd):
  case(e(f=5), UNSUPPORTED, b'feature size 5')
  case(e(f=0), UNSUPPORTED, b'feature size 0')
  case(e(f=5, ptr=None), UNSUPPORTED, b'feature size 5')
  case(e(f=4, **EMPTY), 0)
  case(e(f=1, dtype=_lib.MS_F64, **EMPTY), 0)
case(fwd(f=8), UNSUPPORTED, b'feature size 8')
case(fwd(f=8, cfg=HEUR), UNSUPPORTED, b'feature size 8')
case(bwd(f=8), UNSUPPORTED, b'feature size 8')                               # no heuristics asked for
case(bwd(f=8, cfg=HEUR), UNSUPPORTED, b'feature size 8')                     # asked for, but no buffer
case(bwd(f=8, point_heuristic=P), UNSUPPORTED, b'feature size 8')            # a buffer, but not asked for
case(bwd(f=8, cfg=HEUR, point_heuristic=P, **EMPTY), 0)
case(bwd(f=16, cfg=HEUR, point_heuristic=P, dtype=_lib.MS_F64, **EMPTY), 0)
case(bwd(f=12, cfg=HEUR, point_heuristic=P), UNSUPPORTED, b'feature size 12')
case(bwd(f=17, cfg=HEUR, point_heuristic=P), UNSUPPORTED, b'feature size 17')
case(bwd(cfg=dict(use_alpha_blending=0)), BAD_ARG, b'use_alpha_blending')
case(bwd(cfg=dict(use_alpha_blending=0), ranges=None), BAD_ARG, b'null')     # the null check comes first
case(bwd(cfg=dict(use_alpha_blending=0), **EMPTY), BAD_ARG, b'use_alpha_blending')
case(bwd(grad_points7=None, grad_features=None), 0)                          # no output buffer: nothing to do
case(fwd(cfg=dict(use_alpha_blending=0), **EMPTY), 0)                        # the quantile forward exists

# ---- the moments backward: deterministic needs fixed_exp (-1), blending required (-1), antialias unsupported (-2)
for e in (moments, moments_rows, moments_split):
  case(e(deterministic=1), BAD_ARG, b'fixed_exp')
  case(e(deterministic=1, fixed_exp=P, **EMPTY), 0)
  case(e(cfg=dict(use_alpha_blending=0)), BAD_ARG, b'use_alpha_blending')
  case(e(cfg=dict(antialias=1)), UNSUPPORTED, b'antialias')
  case(e(cfg=dict(antialias=1), **EMPTY), UNSUPPORTED, b'antialias')
  case(e(cfg=dict(antialias=1, use_alpha_blending=0)), BAD_ARG, b'use_alpha_blending')
  case(e(cfg=dict(antialias=1), deterministic=1), BAD_ARG, b'fixed_exp')
  case(e(cfg=dict(antialias=1), w=0), BAD_ARG, b'size')
  # two faults at once: every -1 condition is reported before any -2 condition
  case(e(cfg=dict(tile_size=12 if e is moments else 16, antialias=1, use_alpha_blending=0)), BAD_ARG, b'use_alpha_blending')
  case(e(cfg=dict(tile_size=12 if e is moments else 16, antialias=1), deterministic=1), BAD_ARG, b'fixed_exp')
  case(e(cfg=dict(tile_size=12 if e is moments else 16, antialias=1), h=0), BAD_ARG, b'size')
case(moments_rows(cfg=dict(tile_size=8)), UNSUPPORTED, b'tile')
case(moments_rows(cfg=dict(tile_size=8), deterministic=1), UNSUPPORTED, b'tile')   # before the deterministic check
case(moments_rows(cfg=dict(tile_size=8), **EMPTY), UNSUPPORTED, b'tile')
case(moments_rows(cfg=dict(tile_size=32), **EMPTY), 0)
case(moments(cfg=dict(tile_size=8), **EMPTY), 0)
case(moments_split(cfg=dict(tile_size=12), deterministic=1), UNSUPPORTED, b'tile_size')   # before the deterministic check

# ---- the rows / split forwards serve float32 RGB, plain pdf, blending
for e in (fwd_rows, fwd_split):
  case(e(cfg=dict(antialias=1)), UNSUPPORTED, b'plain pdf')
  case(e(cfg=dict(antialias=1), **EMPTY), UNSUPPORTED, b'plain pdf')
  case(e(cfg=dict(use_alpha_blending=0)), UNSUPPORTED, b'blending')
  case(e(cfg=dict(antialias=1), w=0), UNSUPPORTED, b'plain pdf')             # before the image size

# ---- split scratch: capacity, alignment, parameters
for e, word in ((fwd_split, b'capacity'), (moments_split, b'k_capacity')):
  case(e(k_capacity=-1), BAD_ARG, word)
  case(e(k_capacity=2 ** 31), BAD_ARG, word)
  case(e(k_capacity=2 ** 31 - 1, **EMPTY), 0)
  case(e(scratch=ODD), BAD_ARG, b'aligned')
  case(e(scratch=P + 128), BAD_ARG, b'aligned')
  case(e(scratch=None), BAD_ARG, b'null')
  case(e(min_run=-1), BAD_ARG, b'negative')
  case(e(seg_len=-1), BAD_ARG, b'negative')
  case(e(min_run=512, seg_len=256, **EMPTY), 0)
  case(e(k_capacity=-1, cfg=dict(tile_size=12)), BAD_ARG, word)              # before the configuration

# ---- ms_splat_rows_pack
case(pack(n=-1), BAD_ARG, b'n < 0')
case(pack(n=-1, ptr=None), BAD_ARG, b'n < 0')
case(pack(n=0), 0)
case(pack(n=0, ptr=None), 0)
case(pack(rows=ODD), BAD_ARG, b'aligned')
case(pack(rows=P + 32), BAD_ARG, b'aligned')
case(pack(points7=None), BAD_ARG, b'null')
case(pack(colours=None), BAD_ARG, b'null')
case(pack(rows=None), BAD_ARG, b'null')

# ---- ms_raster_moments_finalize
case(finalize(n=-1), BAD_ARG, b'negative')
case(finalize(deterministic=1), BAD_ARG, b'fixed_exp')
case(finalize(deterministic=1, n=0), BAD_ARG, b'fixed_exp')                  # before the empty call
case(finalize(n=-1, deterministic=1), BAD_ARG, b'negative')
case(finalize(n=0), 0)
case(finalize(n=0, ptr=None), 0)
case(finalize(points7=None), BAD_ARG, b'null')
case(finalize(moments=None), BAD_ARG, b'null')
case(finalize(grad_points7=None, grad_features=None), 0)                     # no output buffer: nothing to do

# ---- empty row window with the required pointers non-null: 0 before any launch
for e in WINDOWED:
  case(e(**EMPTY), 0)
  case(e(row_begin=3, row_end=1), 0)
  case(e(row_begin=4, row_end=9), 0)            # 64 / 16 = 4 tile rows: clamped to [4, 4)
  case(e(row_begin=-5, row_end=0), 0)


@pytest.mark.parametrize("name, args, rc, keyword", CASES)
def test_raster_entry_point_checks_its_arguments(lib, name, args, rc, keyword):
  got = getattr(lib, name)(*args)
  message = lib.ms_last_error_string()
  assert got == rc, (name, got, rc, message)
  if keyword is not None:
    assert keyword in message, (name, keyword, message)


def test_every_raster_entry_point_is_covered():
  covered = {p.values[0] for p in CASES}
  assert covered == {'ms_raster_fwd', 'ms_raster_fwd_split', 'ms_raster_fwd_rows', 'ms_raster_bwd', 'ms_raster_bwd_moments',
                     'ms_raster_bwd_moments_rows', 'ms_raster_bwd_moments_split', 'ms_raster_moments_finalize',
                     'ms_splat_rows_pack'}
