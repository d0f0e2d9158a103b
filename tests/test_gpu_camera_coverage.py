"""``camera_coverage`` on the GPU against the existing per-camera path.

The yardstick is ``project_to_image(gaussians, cameras[c], config)`` for every camera c (the existing suite pins it to
the float64 oracle): its ``indexes`` define the expected bit of every (gaussian, camera) pair, its ``depths`` the
extrema.  It is computed ONCE per (dtype, config) on the full scene of tests/coverage_cases.py (1000 gaussians, 70
cameras) and never modified; every case is a prefix of the gaussians and of the cameras, and takes the matching block
of the yardstick — whether camera c sees gaussian i does not depend on the other rows of either.  The kernel itself runs
on the prefix scene, so that its wave, workgroup and mask-word edges are those of the case.

Non-vacuity is asserted on the yardstick alone, on the full scene and on every case of 63 gaussians or more (a case
of one gaussian cannot hold an unseen and an always-seen one).
"""
import functools
import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from taichi_splatting_amd import (Coverage, RasterConfig, camera_coverage, pack_cameras, render_gaussians, save_ply)
from taichi_splatting_amd.perspective import project_to_image
from tests import coverage_cases as cc

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
F32, F64 = torch.float32, torch.float64
DTYPES = {'f32': F32, 'f64': F64}
CONFIGS = {'default': RasterConfig(), 'other': RasterConfig(blur_cov=0.0, clamp_margin=0.5, alpha_threshold=0.05)}
SHAPES = sorted({(n, 33) for n in (1, 63, 64, 65, 255, 256, 257, 1000)} | {(257, c) for c in (1, 31, 32, 33, 64, 70)})


@functools.lru_cache(maxsize=None)
def yardstick(dt, cfg):
  """(bits (C_MAX, N_MAX) bool, depth (C_MAX, N_MAX) with +inf where not in view, focal (C_MAX,) = max(fx, fy)) from
  project_to_image, camera by camera, on the full scene; shared, never modified"""
  g, cameras = cc.case(cc.N_MAX, cc.C_MAX, DTYPES[dt], DEV)
  bits = torch.zeros((cc.C_MAX, cc.N_MAX), dtype=torch.bool, device=DEV)
  depth = torch.full((cc.C_MAX, cc.N_MAX), float('inf'), dtype=DTYPES[dt], device=DEV)
  for c, camera in enumerate(cameras):
    _, depths, indexes = project_to_image(g, camera, CONFIGS[cfg])
    bits[c, indexes] = True
    depth[c, indexes] = depths[:, 0]
  focal = torch.stack([camera.projection[:2].max() for camera in cameras])
  return bits, depth, focal


def expected(dt, cfg, n, num_cameras):
  bits, depth, focal = (x[:num_cameras] for x in yardstick(dt, cfg))
  bits, depth = bits[:, :n], depth[:, :n]
  rate = torch.where(bits, focal.unsqueeze(1) / depth, torch.zeros_like(depth))     # f_c / z_c, one division in dtype
  words = []
  for first in range(0, num_cameras, 32):
    word = torch.zeros((n,), dtype=torch.int64, device=DEV)
    for b in range(min(32, num_cameras - first)):
      word |= bits[first + b].to(torch.int64) << b
    words.append(word)
  return dict(bits=bits, count=bits.sum(dim=0).to(torch.int32), min_depth=depth.min(dim=0).values,
              max_rate=rate.max(dim=0).values, words=torch.stack(words))


def unsigned(mask):
  """the int32 mask words as non-negative int64"""
  return mask.to(torch.int64) & 0xFFFFFFFF


def same_bits(a, b):
  return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def check_against_yardstick(cov, want, n, num_cameras, dtype):
  assert isinstance(cov, Coverage) and cov.num_cameras == num_cameras
  assert cov.count.dtype == torch.int32 and cov.count.shape == (n,)
  assert cov.max_rate.dtype == dtype and cov.min_depth.dtype == dtype
  assert cov.mask.dtype == torch.int32 and cov.mask.shape == ((num_cameras + 31) // 32, n)
  got_words = unsigned(cov.mask)
  assert torch.equal(got_words, want['words'])                                  # every bit, the unused high bits too
  used = num_cameras % 32
  if used:
    assert int((got_words[-1] >> used).max()) == 0
  for c in sorted({0, num_cameras // 2, num_cameras - 1}):
    assert torch.equal(cov.seen_by(c), want['bits'][c])
  popcount = sum(((got_words >> b) & 1).sum(dim=0) for b in range(32)).to(torch.int32)
  assert torch.equal(cov.count, popcount) and torch.equal(cov.count, want['count'])
  assert torch.equal(cov.seen, want['count'] > 0)
  assert same_bits(cov.min_depth, want['min_depth'])                            # the same pc[2]; +inf where unseen
  unseen = want['count'] == 0
  assert bool(torch.isinf(cov.min_depth[unseen]).all()) and bool((cov.min_depth[unseen] > 0).all())
  assert bool((cov.max_rate[unseen] == 0).all()) and bool((cov.max_rate[~unseen] > 0).all())
  ulp = torch.nextafter(want['max_rate'], torch.full_like(want['max_rate'], float('inf'))) - want['max_rate']
  off = ((cov.max_rate - want['max_rate']).abs() / ulp)[~unseen]
  if off.numel():
    print(f"max_rate: at most {off.max().item():.2f} ulp from torch's division")
    assert off.max().item() <= 2.0


@pytest.mark.parametrize('n, num_cameras', SHAPES)
@pytest.mark.parametrize('dt', DTYPES)
def test_coverage_equals_the_per_camera_path(dt, n, num_cameras):
  want = expected(dt, 'default', n, num_cameras)
  stats = cc.non_vacuous(want['bits'])
  print(f"n {n} C {num_cameras}: {stats}")
  if n >= 63:
    assert 0.1 <= stats['fraction'] <= 0.9 and stats['unseen'] >= 1 and stats['by_all'] >= 1, stats
  g, cameras = cc.case(n, num_cameras, DTYPES[dt], DEV)
  check_against_yardstick(camera_coverage(g, cameras, CONFIGS['default'], masks=True), want, n, num_cameras, DTYPES[dt])


@pytest.mark.parametrize('dt', DTYPES)
def test_full_scene_is_not_vacuous_and_has_every_culling_path(dt):
  bits, depth, _ = yardstick(dt, 'default')
  stats = cc.non_vacuous(bits)
  assert 0.1 <= stats['fraction'] <= 0.9 and stats['unseen'] >= 1 and stats['by_all'] >= 1, stats
  g, cameras = cc.scene()
  assert len({c.image_size for c in cameras}) >= 2 and len({c.depth_range for c in cameras}) >= 2
  assert not bits[:, cc.LOW_ALPHA_ROWS].any() and bits[:, cc.LOW_ALPHA_ROWS].shape[1] == 100    # alpha under the threshold
  assert not bits[:, cc.ZERO_QUAT_ROW].any()                                                    # zero quaternion
  assert not bits[0, list(cc.BEHIND_ROWS)].any() and bits[:, list(cc.BEHIND_ROWS)].any()        # behind camera 0 only
  assert bits[:, cc.ANCHOR].all()
  # geometric culling is real too: an ordinary gaussian that some camera sees and some camera does not
  ordinary = torch.ones(cc.N_MAX, dtype=torch.bool, device=DEV)
  ordinary[cc.LOW_ALPHA_ROWS] = False
  ordinary[cc.ZERO_QUAT_ROW] = False
  partly = bits.any(dim=0) & ~bits.all(dim=0) & ordinary
  assert int(partly.sum()) >= 100


@pytest.mark.parametrize('dt', DTYPES)
def test_non_default_config(dt):
  n, num_cameras = 257, 33
  want = expected(dt, 'other', n, num_cameras)
  assert not torch.equal(want['bits'], expected(dt, 'default', n, num_cameras)['bits'])          # the config matters
  g, cameras = cc.case(n, num_cameras, DTYPES[dt], DEV)
  check_against_yardstick(camera_coverage(g, cameras, CONFIGS['other'], masks=True), want, n, num_cameras, DTYPES[dt])


@pytest.mark.parametrize('dt', DTYPES)
def test_reproducible_and_argument_forms(dt):
  n, num_cameras = 1000, 70
  g, cameras = cc.case(n, num_cameras, DTYPES[dt], DEV)
  with_masks = camera_coverage(g, cameras, masks=True)
  again = camera_coverage(g, cameras, masks=True)
  without = camera_coverage(g, cameras)
  packed = pack_cameras(cameras, DTYPES[dt], DEV)
  assert packed.shape == (num_cameras, 20) and packed.device.type == 'cuda' and packed.dtype == DTYPES[dt]
  from_packed = camera_coverage(g, packed, masks=True)
  # packed cameras of another dtype are cast to the gaussians' (float32 -> float64 -> float32 is exact)
  from_other_dtype = camera_coverage(g, packed.double() if dt == 'f32' else packed.clone(), masks=True)
  assert without.mask is None
  with pytest.raises(ValueError):
    without.seen_by(0)
  for other in (again, without, from_packed, from_other_dtype):
    for name in ('count', 'max_rate', 'min_depth'):
      assert same_bits(getattr(other, name), getattr(with_masks, name)), name
  for other in (again, from_packed, from_other_dtype):
    assert same_bits(other.mask, with_masks.mask)
  # inputs that need detaching and compacting give the same
  wants_grad = g.replace(position=g.position.clone().requires_grad_(True))
  strided = wants_grad.replace(log_scaling=torch.cat([g.log_scaling, g.log_scaling], dim=1)[:, :3])
  assert not strided.log_scaling.is_contiguous()
  assert same_bits(camera_coverage(strided, cameras).min_depth, with_masks.min_depth)
  empty = camera_coverage(g[:0], cameras, masks=True)
  assert empty.count.shape == (0,) and empty.mask.shape == (3, 0)
  with pytest.raises(ValueError):
    camera_coverage(g, packed[:, :19])
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    camera_coverage(g, packed.cpu())


def test_mask_words_past_2_31_elements():
  """words x n = 513 x 4 195 000 > 2^31: the word-major mask is indexed in 64 bits.  The first and the last 32 of the
  16 416 cameras are real; the ones between are a camera whose clip planes coincide (near == far: nobody passes the
  depth test, every wave branches over the projection), so the launch is short.  Word 0 and word 512 — whose first
  element is number 2 147 840 000 of the mask — must equal the single word of a 32-camera call; every word between is
  zero.  The mask is 8.6 GB."""
  copies, words = 4195, 513
  g, cameras = cc.case(cc.N_MAX, 64, F32, DEV)
  n = copies * cc.N_MAX
  assert (words - 1) * n > 2 ** 31
  big = g.apply(lambda t: t.repeat((copies,) + (1,) * (t.ndim - 1)), batch_size=(n,))
  first, last = pack_cameras(cameras[:32], F32, DEV), pack_cameras(cameras[32:], F32, DEV)
  nobody = first[:1].clone()
  nobody[0, 16] = nobody[0, 17] = 1.0
  packed = torch.cat([first, nobody.expand(32 * (words - 2), 20), last]).contiguous()
  assert packed.shape == (32 * words, 20)
  cov = camera_coverage(big, packed, masks=True)
  want_first, want_last = camera_coverage(big, first, masks=True), camera_coverage(big, last, masks=True)
  assert cov.mask.shape == (words, n) and want_first.mask.shape == (1, n)
  assert same_bits(cov.mask[0], want_first.mask[0]) and same_bits(cov.mask[words - 1], want_last.mask[0])
  assert int(want_last.mask[0].ne(0).sum()) > n // 2 and not torch.equal(want_first.mask, want_last.mask)
  assert not bool(cov.mask[1:words - 1].any())
  assert torch.equal(cov.count, want_first.count + want_last.count)
  assert same_bits(cov.min_depth, torch.minimum(want_first.min_depth, want_last.min_depth))
  assert same_bits(cov.max_rate, torch.maximum(want_first.max_rate, want_last.max_rate))
  small = camera_coverage(g, cameras[32:], masks=True)              # and the tiled scene repeats the small one's answer
  assert torch.equal(want_last.mask[0].view(copies, cc.N_MAX), small.mask[0].expand(copies, cc.N_MAX))


def test_captures_into_a_graph():
  """no allocation of its own beyond torch's, no host read, no synchronisation: captured once, replayed after the
  gaussians moved in place, equal to an eager call on the moved scene"""
  n, num_cameras = 1000, 70
  g, cameras = cc.case(n, num_cameras, F32, DEV)
  g = g.replace(position=g.position.clone())
  packed = pack_cameras(cameras, F32, DEV)
  before = camera_coverage(g, packed, masks=True)                  # (also loads the library outside the capture)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    static = camera_coverage(g, packed, masks=True)
  g.position.add_(torch.tensor([0.05, -0.02, 0.03], device=DEV))
  graph.replay()
  torch.cuda.synchronize()
  eager = camera_coverage(g, packed, masks=True)
  assert not torch.equal(eager.mask, before.mask)                  # the move changed the answer
  for name in ('count', 'max_rate', 'min_depth', 'mask'):
    assert same_bits(getattr(static, name), getattr(eager, name)), name


@pytest.mark.parametrize('dt', DTYPES)
def test_filter_sigma_baked_into_the_gpu_scene(dt):
  n, num_cameras = 1000, 70
  g, cameras = cc.case(n, num_cameras, DTYPES[dt], DEV)
  cov = camera_coverage(g, cameras)
  sigma = cov.filter_sigma()
  assert sigma.dtype == DTYPES[dt] and sigma.device.type == 'cuda'
  assert torch.equal(sigma == 0, ~cov.seen)
  seen = cov.seen
  assert torch.allclose(sigma[seen].double() * cov.max_rate[seen].double(), torch.full((int(seen.sum()),), 0.2 ** 0.5,
                                                                                         dtype=F64, device=DEV), rtol=1e-6)
  out = g.with_filter_3d(sigma)
  assert out.log_scaling.device.type == 'cuda'
  keep = cc.check_filtered(g, sigma, out, DTYPES[dt])
  assert torch.equal(keep, ~cov.seen.cpu()) and 100 <= int(keep.sum()) < n


def test_zero_filter_renders_the_same_image():
  g, cameras = cc.case(1000, 2, F32, DEV)
  unfiltered = g.with_filter_3d(torch.zeros(1000, device=DEV))
  for name in ('log_scaling', 'alpha_logit'):
    assert same_bits(getattr(unfiltered, name), getattr(g, name))
  with torch.no_grad():
    for camera in cameras:
      a = render_gaussians(g, camera, RasterConfig()).image
      b = render_gaussians(unfiltered, camera, RasterConfig()).image
      assert float(a.abs().max()) > 0.1 and same_bits(a, b)
    filtered = g.with_filter_3d(torch.full((1000,), 0.05, device=DEV))       # (and a real filter changes the image)
    assert not torch.equal(render_gaussians(filtered, cameras[-1], RasterConfig()).image, a)


def test_render_scene_tool_reports_the_coverage(tmp_path):
  """``tools/render_scene.py scene.ply --coverage``, a fresh child process: the histogram sums to n"""
  n = 257
  g, _ = cc.scene()
  g = g[:n]
  g = g.replace(feature=torch.cat([(g.feature.unsqueeze(2) - 0.5) / 0.28209479177387814, torch.zeros(n, 3, 3)], dim=2))
  save_ply(g, tmp_path / 'scene.ply')
  tool = str(Path(__file__).resolve().parent.parent / 'tools' / 'render_scene.py')
  done = subprocess.run([sys.executable, tool, str(tmp_path / 'scene.ply'), '--coverage', '--views', '3', '--size', '64', '48'],
                        capture_output=True, text=True, timeout=120)
  assert done.returncode == 0, done.stderr[-2000:]
  report = json.loads(done.stdout.strip().splitlines()[-1])
  coverage = report['coverage']
  assert report['n'] == n and coverage['views'] == 3 and coverage['ms'] > 0
  assert coverage['seen_by_none'] + coverage['seen_by_some'] + coverage['seen_by_all'] == n
  assert coverage['seen_by_none'] >= 26                            # the low-alpha tenth and the zero quaternion
  assert 'coverage: 3 views' in done.stderr
