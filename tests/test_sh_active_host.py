"""Active SH degree, host side (no GPU): the C-ABI declares the two entry points and the descriptor field, a zeroed
descriptor means "every stored band", the library refuses a band count the scene does not store, and the Python surface
validates ``sh_degree`` / ``active_degree`` before anything asks for a device."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from taichi_splatting_amd import Gaussians3D, RasterConfig, _lib, evaluate_sh_at, render_gaussians
from taichi_splatting_amd.testing import random_camera

HEADER = (Path(__file__).resolve().parent.parent / 'include' / 'mi355_splat.h').read_text()


def test_header_declares_the_active_degree_abi():
  for name in ('ms_sh_fwd_active', 'ms_sh_bwd_active'):
    decl = re.search(rf'\bint {name}\(([^;]*)\);', HEADER)
    assert decl is not None, name
    assert 'int degree, int active_degree' in decl.group(1), (name, decl.group(1))
    assert name in _lib.SIGNATURES
  desc = re.search(r'typedef struct ms_frame_desc \{(.*?)\} ms_frame_desc;', HEADER, re.S).group(1)
  fields = re.findall(r'^\s*(?:u?int\d+_t|double|ms_raster_config)\s+([^;]+);', desc, re.M)
  names = [n.strip() for f in fields for n in f.split(',')]
  assert names[names.index('split_seg_len') + 1] == 'sh_active_bands', names      # behind split_seg_len
  assert re.search(r'#define MS_VERSION 501\b', HEADER)


def test_zeroed_descriptor_means_all_bands():
  desc = _lib.FrameDescC()
  assert desc.sh_active_bands == 0
  raw = (ctypes.c_char * ctypes.sizeof(_lib.FrameDescC))()
  assert ctypes.cast(raw, ctypes.POINTER(_lib.FrameDescC)).contents.sh_active_bands == 0
  assert [n for n, _ in _lib.FrameDescC._fields_].index('sh_active_bands') == \
    [n for n, _ in _lib.FrameDescC._fields_].index('split_seg_len') + 1


def _desc(sh_degree, bands):
  from taichi_splatting_amd import frame
  desc, _ = frame.frame_desc(100, (64, 48), torch.float32, 3, sh_degree, RasterConfig())
  desc.sh_active_bands = bands
  return desc


def test_layout_query_refuses_bands_the_scene_does_not_store():
  if not _lib.LIB_PATH.exists():
    pytest.skip("libmi355_splat.so is not built")
  lib, lay = _lib.load(), _lib.FrameLayoutC()
  bad_arg = -1
  for sh_degree, bands, want in ((3, 0, 0), (3, 1, 0), (3, 4, 0), (3, 5, bad_arg), (1, 2, 0), (1, 3, bad_arg), (0, 2, bad_arg),
                                 (-1, 0, 0), (-1, 1, bad_arg), (2, -1, bad_arg)):
    desc = _desc(sh_degree, bands)
    assert lib.ms_frame_layout_query(ctypes.byref(desc), ctypes.byref(lay)) == want, (sh_degree, bands)
    if want:
      assert b'sh_active_bands' in lib.ms_last_error_string()


def test_frame_desc_carries_the_active_degree():
  from taichi_splatting_amd import frame
  for active, bands in ((None, 0), (0, 1), (2, 3), (3, 4)):
    desc, _ = frame.frame_desc(10, (64, 48), torch.float32, 3, 3, RasterConfig(), active_degree=active)
    assert desc.sh_active_bands == bands


def _scene(n, degree):
  torch.manual_seed(0)
  q = torch.nn.functional.normalize(torch.randn(n, 4), dim=1)
  return Gaussians3D(position=torch.randn(n, 3), log_scaling=torch.zeros(n, 3), rotation=q, alpha_logit=torch.zeros(n, 1),
                     feature=torch.randn(n, 3, (degree + 1) ** 2), batch_size=(n,))


@pytest.mark.parametrize('stored,sh_degree', [(3, 4), (1, 2), (3, True), (3, -1), (3, 1.0)])
def test_render_gaussians_validates_sh_degree_before_any_device_check(stored, sh_degree):
  cam = random_camera(image_size=(64, 48))
  with pytest.raises(ValueError, match='sh_degree'):
    render_gaussians(_scene(20, stored), cam, RasterConfig(), use_sh=True, sh_degree=sh_degree)


def test_render_gaussians_refuses_sh_degree_without_sh():
  cam = random_camera(image_size=(64, 48))
  g = _scene(20, 0)
  g = g.replace(feature=g.feature[:, :, 0])
  with pytest.raises(ValueError, match='use_sh'):
    render_gaussians(g, cam, RasterConfig(), use_sh=False, sh_degree=0)


@pytest.mark.parametrize('stored,active', [(3, 4), (1, 2), (3, True), (3, -1)])
def test_evaluate_sh_at_validates_active_degree_before_any_device_check(stored, active):
  g = _scene(20, stored)
  with pytest.raises(ValueError, match='active_degree'):
    evaluate_sh_at(g.feature, g.position, torch.arange(20), torch.zeros(3), active_degree=active)
