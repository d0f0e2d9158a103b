"""bench.py's line and its --dump-outputs files: a plain run times the frames and nothing else, --full adds the secondary
measurements, and the dumped arrays are what the last timed step computed."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
SMALL = ['--n', '200000', '--size', '512', '--steps', '3', '--warmup', '1']
EXTRAS = ('graph_ms_per_step', 'lazy_settle', 'tile_sweep_ms', 'roofline', 'frame', 'extra', 'cpu_baseline')


def run_bench(*extra):
  proc = subprocess.run([sys.executable, str(ROOT / 'bench.py'), *SMALL, *extra], capture_output=True, text=True,
                        timeout=900)
  assert proc.returncode == 0, proc.stderr[-3000:]
  lines = [l for l in proc.stdout.splitlines() if l.startswith('{')]
  assert len(lines) == 1, proc.stdout
  return json.loads(lines[0])


def test_dump_samples_are_fixed_and_bounded(tmp_path):
  sys.path.insert(0, str(ROOT))
  import bench
  h, w, n = 1200, 1000, 300_000            # above both sample sizes (2^20 pixels, 65 536 gaussians)
  torch.manual_seed(0)
  arrays = {'image': torch.rand(h, w, 3), 'image_weight': torch.rand(h, w)}
  for name, shape in zip(bench.LEAF_NAMES, [(3,), (3,), (4,), (1,), (3, 16)]):
    arrays['grad_' + name] = torch.randn(n, *shape, dtype=torch.float64 if name == 'rotation' else torch.float32)
  bench.write_outputs(tmp_path / 'a', arrays)
  bench.write_outputs(tmp_path / 'b', arrays)
  files = sorted(p.name for p in (tmp_path / 'a').iterdir())
  assert files == sorted(f'{k}.npy' for k in arrays)
  total = 0
  for f in files:
    a, b = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
    assert np.array_equal(a, b), f
    assert a.dtype == (np.float64 if f == 'grad_rotation.npy' else np.float32), f
    total += a.nbytes
  assert total <= 64 << 20
  # the gaussian rows are one sample, shared by the five gradients, in ascending order
  assert np.load(tmp_path / 'a' / 'image.npy').shape == (1 << 20, 3)
  pos = np.load(tmp_path / 'a' / 'grad_position.npy')
  assert pos.shape == (65536, 3)
  rows = arrays['grad_position'].numpy()
  idx = [int(np.flatnonzero((rows[:, 0] == r[0]) & (rows[:, 1] == r[1]))[0]) for r in pos[:50]]
  assert idx == sorted(idx)
  assert np.array_equal(np.load(tmp_path / 'a' / 'grad_alpha_logit.npy')[:50], arrays['grad_alpha_logit'].numpy()[idx])

  # arrays within the sample size are written whole, in order
  small = {'image': torch.rand(16, 8, 3), 'grad_position': torch.randn(10, 3)}
  bench.write_outputs(tmp_path / 'c', small)
  assert np.array_equal(np.load(tmp_path / 'c' / 'image.npy'), small['image'].reshape(-1, 3).numpy())
  assert np.array_equal(np.load(tmp_path / 'c' / 'grad_position.npy'), small['grad_position'].numpy())


@pytest.mark.gpu
def test_plain_run_times_the_frames_and_dumps_the_last_step(tmp_path):
  out = run_bench('--dump-outputs', str(tmp_path))
  for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
    assert key in out, key
  assert out['steps'] == 3 and out['ms_per_step'] > 0 and out['value'] > 0
  assert not [k for k in EXTRAS if k in out], out.keys()

  # 512 x 512 pixels: the image is written whole; it is what one frame of the same scene renders
  sys.path.insert(0, str(ROOT))
  import bench
  from taichi_splatting_amd import RasterConfig, render_gaussians
  scene_args = type('Args', (), dict(seed=0, size=512, height=None, n=200000, sh_degree=3))()
  g, cam = bench.make_scene(scene_args, torch.device('cuda', 0))
  with torch.no_grad():
    r = render_gaussians(g, cam, RasterConfig(tile_size=16, pixel_stride=(2, 2)), use_sh=True)
  image = np.load(tmp_path / 'image.npy')
  assert image.dtype == np.float32 and image.shape == (512 * 512, 3)
  np.testing.assert_allclose(image, r.image.reshape(-1, 3).cpu().numpy(), rtol=0, atol=1e-5)
  np.testing.assert_allclose(np.load(tmp_path / 'image_weight.npy'), r.image_weight.reshape(-1).cpu().numpy(), rtol=0, atol=1e-5)
  for name in bench.LEAF_NAMES:        # 200 000 gaussians: a sample of 65 536 rows
    grad = np.load(tmp_path / f'grad_{name}.npy')
    assert grad.dtype == np.float32 and grad.shape[0] == 65536 and np.isfinite(grad).all() and np.abs(grad).max() > 0, name


@pytest.mark.gpu
def test_full_run_adds_the_secondary_measurements():
  out = run_bench('--full', '--no-cpu-baseline')
  assert out['steps'] == 3 and out['ms_per_step'] > 0
  assert out['graph_ms_per_step'] and out['lazy_settle']['ms_per_step'] > 0
  assert set(out['tile_sweep_ms']) == {'8', '16', '32'}
  assert out['frame']['stage_ms']['raster_bwd'] > 0 and out['roofline']['kernel_ms'] > 0
  assert 'iteration_ms_reference_loop' in out['extra']['train_step']
