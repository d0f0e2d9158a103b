"""No GPU: the host side of camera-set coverage — ``pack_cameras``' layout, the ``Coverage`` accessors on hand-made
tensors, ``Gaussians3D.with_filter_3d`` against its formulas written out here in float64, and the argument checks of
``ms_camera_coverage`` (they come before any launch)."""
import functools
import math
import subprocess
import sys

import pytest
import torch

from taichi_splatting_amd import CameraParams, Coverage, RasterConfig, _lib, camera_coverage, pack_cameras
from taichi_splatting_amd.testing.random_data import random_camera
from tests.coverage_cases import check_filtered, filter_scene

F32, F64 = torch.float32, torch.float64


# ---- pack_cameras ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def two_cameras():
  """two cameras with different image sizes and clip planes (shared: never modified)"""
  torch.manual_seed(11)
  a = random_camera(image_size=(320, 200), near_plane=0.1)
  b = random_camera(image_size=(97, 131), near_plane=0.37)
  b.far_plane = 55.5
  return a, b


def test_pack_cameras_layout_value_by_value():
  cameras = two_cameras()
  packed = pack_cameras(cameras, F32)
  assert packed.shape == (2, 20) and packed.dtype == F32 and packed.is_contiguous() and not packed.requires_grad
  assert packed.device == cameras[0].T_camera_world.device
  assert _lib.COVERAGE_CAMERA_VALUES == 20
  for row, c in zip(packed, cameras):
    for i in range(3):
      for j in range(4):
        assert row[i * 4 + j].item() == c.T_camera_world[i, j].item(), (i, j)
    for k in range(4):
      assert row[12 + k].item() == c.projection[k].item(), k
    assert row[16].item() == torch.tensor(c.near_plane, dtype=F32).item()
    assert row[17].item() == torch.tensor(c.far_plane, dtype=F32).item()
    assert row[18].item() == c.image_size[0] and row[19].item() == c.image_size[1]
  assert packed[0, 16].item() != packed[1, 16].item() and packed[0, 17].item() != packed[1, 17].item()
  assert packed[0, 18].item() != packed[1, 18].item() and packed[0, 19].item() != packed[1, 19].item()


def test_pack_cameras_casts_and_detaches():
  cameras = two_cameras()
  packed = pack_cameras(cameras, F64)
  assert packed.dtype == F64
  assert torch.equal(packed[:, :16], pack_cameras(cameras, F32)[:, :16].double())      # float32 camera tensors, widened
  assert packed[1, 16].item() == 0.37 and packed[1, 17].item() == 55.5                 # host numbers rounded once
  assert pack_cameras(cameras, F32)[1, 16].item() == torch.tensor(0.37, dtype=F32).item()
  wants_grad = CameraParams(projection=cameras[0].projection.clone().requires_grad_(True),
                            T_camera_world=cameras[0].T_camera_world.clone().requires_grad_(True),
                            near_plane=0.1, far_plane=10.0, image_size=(8, 8))
  assert not pack_cameras([wants_grad], F32).requires_grad


def test_pack_cameras_refuses_empty_and_oversized_sets():
  with pytest.raises(ValueError):
    pack_cameras([], F32)
  with pytest.raises(ValueError):
    pack_cameras([two_cameras()[0]] * 65536, F32)
  assert pack_cameras(iter(two_cameras()), F32).shape == (2, 20)                       # any iterable, read once


# ---- Coverage ----------------------------------------------------------------------------------------------------------

def hand_made(masks=True):
  """four gaussians, C = 33: gaussian 0 unseen; 1 seen by camera 0; 2 by cameras 31 and 32; 3 by all 33"""
  word0 = torch.tensor([0, 1, -2 ** 31, -1], dtype=torch.int32)                       # bit 31 is the int32 sign bit
  word1 = torch.tensor([0, 0, 1, 1], dtype=torch.int32)
  return Coverage(count=torch.tensor([0, 1, 2, 33], dtype=torch.int32),
                  max_rate=torch.tensor([0.0, 100.0, 250.0, 40.0], dtype=F64),
                  min_depth=torch.tensor([math.inf, 2.0, 1.5, 8.0], dtype=F64),
                  mask=torch.stack([word0, word1]) if masks else None, num_cameras=33)


def test_coverage_seen_and_seen_by():
  cov = hand_made()
  assert cov.seen.tolist() == [False, True, True, True] and cov.seen.dtype == torch.bool
  assert cov.seen_by(0).tolist() == [False, True, False, True]
  assert cov.seen_by(1).tolist() == [False, False, False, True]
  assert cov.seen_by(31).tolist() == [False, False, True, True]
  assert cov.seen_by(32).tolist() == [False, False, True, True]                        # bit 0 of the LAST word
  assert cov.seen_by(32).dtype == torch.bool and cov.seen_by(32).shape == (4,)
  popcount = sum(cov.seen_by(c).to(torch.int32) for c in range(33))
  assert torch.equal(popcount, cov.count)
  for bad in (33, -1, 64, 1.0, True):
    with pytest.raises(IndexError):
      cov.seen_by(bad)
  with pytest.raises(ValueError, match="masks=True"):
    hand_made(masks=False).seen_by(0)


def test_coverage_filter_sigma():
  cov = hand_made()
  sigma = cov.filter_sigma()
  assert sigma.dtype == F64 and sigma[0].item() == 0.0
  want = [math.sqrt(0.2) / r for r in (100.0, 250.0, 40.0)]
  assert all(abs(s - w) <= 1e-15 * w for s, w in zip(sigma[1:].tolist(), want))
  assert abs(cov.filter_sigma(0.5)[2].item() - math.sqrt(0.5) / 250.0) <= 1e-17
  assert cov.filter_sigma(0.0).tolist() == [0.0] * 4
  with pytest.raises(ValueError):
    cov.filter_sigma(-1.0)


# ---- Gaussians3D.with_filter_3d ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [F64, F32], ids=['f64', 'f32'])
def test_with_filter_3d_matches_the_formulas(dtype):
  g, sigma = filter_scene(200, dtype)
  out = g.with_filter_3d(sigma)
  keep = check_filtered(g, sigma, out, dtype)
  assert int(keep.sum()) == 67 and (out.log_scaling[~keep] - g.log_scaling[~keep]).max().item() > 0.5
  assert out.position is g.position and out.rotation is g.rotation and out.feature is g.feature
  alpha_range = torch.sigmoid(g.alpha_logit.double())
  assert alpha_range.min().item() >= 0.0099 and alpha_range.max().item() <= 0.9901


def test_with_filter_3d_gradcheck():
  g, sigma = filter_scene(5, F64, seed=9)
  assert (sigma == 0).sum().item() == 2

  def filtered(log_scaling, alpha_logit):
    out = g.replace(log_scaling=log_scaling, alpha_logit=alpha_logit).with_filter_3d(sigma)
    return out.log_scaling, out.alpha_logit

  inputs = (g.log_scaling.clone().requires_grad_(True), g.alpha_logit.clone().requires_grad_(True))
  assert torch.autograd.gradcheck(filtered, inputs, eps=1e-6, atol=1e-8, rtol=1e-6)
  a, b = filtered(*inputs)
  (a.sum() + b.sum()).backward()
  assert all(x.grad is not None and bool(torch.isfinite(x.grad).all()) and x.grad.abs().sum().item() > 0 for x in inputs)


def test_with_filter_3d_refuses_bad_sigmas():
  g, sigma = filter_scene(6, F32)
  bad = [sigma[:5], sigma.unsqueeze(1), sigma.reshape(2, 3), sigma.tolist(), None]
  for value, entry in ((-1e-3, 1), (math.nan, 2), (math.inf, 4)):
    s = sigma.clone()
    s[entry] = value
    bad.append(s)
  for s in bad:
    with pytest.raises(ValueError):
      g.with_filter_3d(s)
  assert torch.equal(g.with_filter_3d(torch.zeros(6)).log_scaling, g.log_scaling)


# ---- ms_camera_coverage: argument checks --------------------------------------------------------------------------------

NAMES = ('position', 'log_scaling', 'rotation', 'alpha_logit', 'cameras', 'count', 'max_rate', 'min_depth', 'mask')


def call(lib, *, n=10, num_cameras=4, dtype=_lib.MS_F32, **pointers):
  """ms_camera_coverage with dummy non-null pointers (8: aligned for both dtypes): a rejected call launches nothing,
  and n == 0 returns before one"""
  p = {name: pointers.get(name, 8) for name in NAMES}
  return lib.ms_camera_coverage(p['position'], p['log_scaling'], p['rotation'], p['alpha_logit'], p['cameras'],
                                num_cameras, 0.3, 0.15, 1 / 255., n, p['count'], p['max_rate'], p['min_depth'], p['mask'],
                                dtype, None)


def test_camera_coverage_argument_errors(lib):
  assert call(lib, n=-1) == -1 and b'n >= 0' in lib.ms_last_error_string()
  assert call(lib, n=2 ** 31) == -1 and b'2^31' in lib.ms_last_error_string()
  assert call(lib, n=2 ** 40) == -1
  for c in (0, -1, 65536, 1 << 20):
    assert call(lib, num_cameras=c) == -1, c
    assert b'num_cameras' in lib.ms_last_error_string()
  for name in NAMES[:8]:                                                              # every required pointer
    assert call(lib, **{name: None}) == -1, name
    assert b'null' in lib.ms_last_error_string()
  for dtype in (7, -1, 2):
    assert call(lib, dtype=dtype) == -1 and b'dtype' in lib.ms_last_error_string()
  for name in NAMES:                                                                  # misaligned, the mask included
    assert call(lib, **{name: 10}) == -1, name
    assert b'aligned' in lib.ms_last_error_string()
  for name in NAMES[:5] + NAMES[6:8]:                                                 # a double array at a 4-byte address
    assert call(lib, dtype=_lib.MS_F64, **{name: 12}) == -1, name
    assert b'aligned' in lib.ms_last_error_string()
  # every argument is checked, also with nothing to do
  assert call(lib, n=0, num_cameras=0) == -1 and call(lib, n=0, dtype=7) == -1 and call(lib, n=0, position=2) == -1
  assert call(lib, n=0) == 0 and call(lib, n=0, dtype=_lib.MS_F64) == 0
  assert call(lib, n=0, mask=None) == 0 and call(lib, n=0, num_cameras=65535) == 0
  assert call(lib, n=0, **{name: None for name in NAMES}) == 0                        # what empty tensors hand over
  header = (_lib.PACKAGE_DIR.parent / 'include' / 'mi355_splat.h').read_text()
  assert '#define MS_COVERAGE_CAMERA_VALUES 20' in header and '#define MS_COVERAGE_MAX_CAMERAS 65535' in header
  assert _lib.COVERAGE_MAX_CAMERAS == 65535


def test_camera_coverage_has_no_cpu_fallback():
  g, _ = filter_scene(4, F32)
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    camera_coverage(g, list(two_cameras()), RasterConfig())
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    camera_coverage(g, pack_cameras(two_cameras(), F32))


def test_render_scene_help_lists_coverage():
  tool = _lib.PACKAGE_DIR.parent / 'tools' / 'render_scene.py'
  done = subprocess.run([sys.executable, str(tool), '--help'], capture_output=True, text=True, timeout=120)
  assert done.returncode == 0 and '--coverage' in done.stdout, done.stderr[-500:]
