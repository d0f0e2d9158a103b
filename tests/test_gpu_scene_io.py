"""scene_io on the GPU: a scene saved from device tensors and loaded back onto the device is the same scene, field by
field and pixel by pixel.

One scene for the whole module: ``random_3d_gaussians`` at N = 257 (one past a block of 256) with degree-3 coefficients,
saved once.  "Same" is ``torch.equal`` on every field, on the image and on everything the frame computes per visible
gaussian (the visible set ``points.idx``, depths, projected gaussians, colours): all of that is deterministic.  The
per-gaussian visibility SUMS are accumulated with float atomics across waves and tiles, so two renders of the very same
tensors may differ in the last bits; they are compared at the tolerance tests/test_gpu_frame.py uses for them.
"""
import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from taichi_splatting_amd import RasterConfig, load_ply, render_gaussians, save_ply
from taichi_splatting_amd.testing import random_3d_gaussians, random_camera

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
DEV = 'cuda:0'
N = 257
SIZE = (64, 48)
FIELDS = ('position', 'log_scaling', 'rotation', 'alpha_logit', 'feature')


@pytest.fixture(scope='module')
def saved(tmp_path_factory):
  """(scene on the GPU, camera on the GPU, path of its file): made once, never written to"""
  torch.manual_seed(3)
  camera = random_camera(image_size=SIZE)
  scene = random_3d_gaussians(N, camera, scale_factor=1.0, alpha_range=(0.1, 0.9))
  scene = scene.replace(feature=(torch.rand(N, 3, 16) - 0.5) * 0.5).to(DEV)
  path = tmp_path_factory.mktemp('scene_io') / 'scene.ply'
  save_ply(scene, path)
  return scene, camera.to(device=DEV), path


def assert_same_scene(a, b):
  for key in FIELDS:
    x, y = getattr(a, key), getattr(b, key)
    assert x.device == y.device and x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), key


def test_saved_and_loaded_scene_renders_the_same_image(saved):
  scene, camera, path = saved
  loaded = load_ply(path, device='cuda')
  assert loaded.position.is_cuda and loaded.feature.shape == (N, 3, 16) and tuple(loaded.batch_size) == (N,)
  assert_same_scene(loaded, scene)
  config = RasterConfig(compute_visibility=True)
  with torch.no_grad():
    want = render_gaussians(scene, camera, config, use_sh=True)
    got = render_gaussians(loaded, camera, config, use_sh=True)
  assert want.image.shape == (SIZE[1], SIZE[0], 3) and float(want.image.abs().sum()) > 0.0
  assert torch.equal(got.image, want.image) and torch.equal(got.image_weight, want.image_weight)
  assert want.points.idx.shape[0] > N // 2                                # most of the scene is in view
  assert torch.equal(got.points.idx, want.points.idx)                      # the same visible set
  for key in ('depths', 'gaussians2d', 'features'):
    assert torch.equal(getattr(got.points, key), getattr(want.points, key)), key
  assert float(want.points.visibility.sum()) > 0.0
  assert torch.allclose(got.points.visibility, want.points.visibility, rtol=1e-4, atol=1e-5)


def test_cpu_and_gpu_saves_are_byte_identical(saved, tmp_path):
  scene, _, path = saved
  from_cpu = tmp_path / 'from_cpu.ply'
  save_ply(scene.cpu(), from_cpu, chunk_rows=100)
  assert from_cpu.read_bytes() == path.read_bytes()
  assert_same_scene(load_ply(path), scene.cpu())


def test_small_slabs_through_the_reused_staging_buffer(saved):
  scene, _, path = saved
  whole = load_ply(path, device='cuda', chunk_rows=1 << 20)
  slabs = load_ply(path, device='cuda', chunk_rows=100)                    # 100 + 100 + 57 rows through one pinned buffer
  assert_same_scene(slabs, whole)
  assert_same_scene(slabs, scene)
  low = load_ply(path, device=DEV, sh_degree=1, chunk_rows=100)
  assert torch.equal(low.feature, scene.feature[:, :, :4])


def test_render_scene_tool(saved, tmp_path):
  _, _, path = saved
  out = tmp_path / 'views'
  done = subprocess.run([sys.executable, str(ROOT / 'tools' / 'render_scene.py'), str(path), '--views', '2', '--size', '64', '48',
                         '--out', str(out)], capture_output=True, text=True, timeout=120)
  assert done.returncode == 0, done.stderr[-2000:]
  report = json.loads(done.stdout.strip().splitlines()[-1])
  assert report['n'] == N and report['sh_degree'] == 3 and report['views'] == 2
  assert len(report['visible']) == 2 and len(report['overlaps']) == 2 and report['frame_ms'] > 0.0
  for key in ('read_s', 'upload_ms', 'unpack_ms', 'load_s'):
    assert report[key] >= 0.0
  assert sorted(p.name for p in out.iterdir()) == ['view_000.npy', 'view_001.npy']
