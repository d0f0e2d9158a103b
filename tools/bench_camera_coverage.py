#!/usr/bin/env python
"""camera_coverage (csrc/camera_coverage.hip) against the per-camera loop it replaces, same process, same box.

Scene: N random gaussians (6 M) in a unit ball, float32; C in {16, 64, 256} pinhole cameras (1024 x 768, 60 degrees
across the width) on a circle of radius 0.8 INSIDE the cloud, looking at its centre, so that every camera culls a real
share of the scene by depth and by frustum (the in-view share of all pairs is printed).  Per C, with and without the
per-camera masks, device time from events around the call, median over the rounds after warm-up, variants alternating
inside a round:

    kernel, packed    camera_coverage(g, packed (C, 20) tensor): the one launch, what a captured graph replays
    kernel, list      camera_coverage(g, [CameraParams] * C): the same behind pack_cameras (stack, cast, one small copy)
    loop              for every camera: project_to_image (project kernel, scan, host read of the visible count, gather),
                      count[idx] += 1, scatter_reduce_ amin / amax for the depth and the rate, and the mask bit — the
                      composition the package offered before, on its unchanged code paths

The three results are compared first: count, min_depth and the masks must be equal, max_rate within float32 rounding.

    python tools/bench_camera_coverage.py [--rows 6000000] [--cameras 16 64 256] [--rounds 10] [--loop-rounds 3]
"""
import argparse
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from taichi_splatting_amd import CameraParams, Gaussians3D, RasterConfig, camera_coverage, pack_cameras   # noqa: E402
from taichi_splatting_amd.perspective import project_to_image                                              # noqa: E402


def make_scene(n, device):
  gen = torch.Generator(device=device).manual_seed(n)
  r = lambda *shape: torch.randn(*shape, device=device, generator=gen)
  direction = r(n, 3)
  radius = torch.rand(n, 1, device=device, generator=gen) ** (1.0 / 3.0)
  return Gaussians3D(position=direction / direction.norm(dim=1, keepdim=True) * radius, log_scaling=0.5 * r(n, 3) - 5.0,
                     rotation=r(n, 4), alpha_logit=2.0 * r(n, 1), feature=torch.rand(n, 3, device=device, generator=gen),
                     batch_size=(n,))


def ring_cameras(views, device, radius=0.8, size=(1024, 768)):
  w, h = size
  focal = 0.5 * w / math.tan(math.radians(30.0))
  projection = torch.tensor([focal, focal, 0.5 * w, 0.5 * h], dtype=torch.float32, device=device)
  down = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
  cameras = []
  for v in range(views):
    angle = 2.0 * math.pi * v / views
    eye = radius * torch.tensor([math.sin(angle), 0.0, -math.cos(angle)], dtype=torch.float64)
    forward = -eye / eye.norm()
    right = torch.linalg.cross(down, forward)
    right = right / right.norm()
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3] = torch.stack([right, torch.linalg.cross(forward, right), forward])
    T[:3, 3] = -T[:3, :3] @ eye
    cameras.append(CameraParams(projection=projection, T_camera_world=T.to(torch.float32).to(device), near_plane=0.05,
                                far_plane=50.0, image_size=(w, h), id=v))
  return cameras


def loop_coverage(g, cameras, config, masks):
  """the composition camera_coverage replaces: one projection, one host read and three or four scatters per camera"""
  n, device = g.position.shape[0], g.position.device
  count = torch.zeros((n,), dtype=torch.int32, device=device)
  max_rate = torch.zeros((n,), dtype=g.position.dtype, device=device)
  min_depth = torch.full((n,), float('inf'), dtype=g.position.dtype, device=device)
  mask = torch.zeros(((len(cameras) + 31) // 32, n), dtype=torch.int32, device=device) if masks else None
  for c, camera in enumerate(cameras):
    _, depths, idx = project_to_image(g, camera, config)
    z = depths[:, 0]
    count[idx] += 1
    min_depth.scatter_reduce_(0, idx, z, 'amin')
    max_rate.scatter_reduce_(0, idx, camera.projection[:2].max() / z, 'amax')
    if masks:
      bit = 1 << (c % 32)
      row = mask[c // 32]
      row[idx] = row[idx] | (bit - (1 << 32) if bit >= 1 << 31 else bit)
  return count, max_rate, min_depth, mask


def timed(fn):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  out = fn()
  end.record()
  end.synchronize()
  return out, start.elapsed_time(end)


def summary(xs):
  return f"median {statistics.median(xs):9.3f} ms  min {min(xs):9.3f}  max {max(xs):9.3f}  ({len(xs)} rounds)"


def main():
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--rows', type=int, default=6_000_000)
  p.add_argument('--cameras', type=int, nargs='+', default=[16, 64, 256])
  p.add_argument('--rounds', type=int, default=10, help="timed rounds of the kernel variants")
  p.add_argument('--loop-rounds', type=int, default=3, help="timed rounds of the per-camera loop")
  p.add_argument('--warmup', type=int, default=2)
  args = p.parse_args()
  if not torch.cuda.is_available():
    sys.exit("bench_camera_coverage: no GPU visible (there is no CPU fallback to time)")
  device = torch.device('cuda:0')
  n, config = args.rows, RasterConfig()
  g = make_scene(n, device)
  torch.cuda.synchronize()
  print(f"{torch.cuda.get_device_name(device)}; torch {torch.__version__}; N = {n}, float32, cameras 1024 x 768")

  for views in args.cameras:
    cameras = ring_cameras(views, device)
    packed = pack_cameras(cameras, torch.float32, device)

    cov = camera_coverage(g, packed, config, masks=True)
    count, max_rate, min_depth, mask = loop_coverage(g, cameras, config, True)
    assert torch.equal(cov.count, count) and torch.equal(cov.mask, mask) and torch.equal(cov.min_depth, min_depth)
    assert torch.allclose(cov.max_rate, max_rate, rtol=3e-7, atol=0.0)
    share = float(count.double().mean()) / views
    print(f"\nC = {views}: {share:.1%} of all (gaussian, camera) pairs in view; seen by 0 / all: "
          f"{int((count == 0).sum())} / {int((count == views).sum())}; kernel and loop agree")
    del cov, count, max_rate, min_depth, mask

    for masks in (False, True):
      times = dict(packed=[], listed=[], loop=[])
      for r in range(args.warmup + args.rounds):
        _, ms_packed = timed(lambda: camera_coverage(g, packed, config, masks=masks))
        _, ms_listed = timed(lambda: camera_coverage(g, cameras, config, masks=masks))
        if r >= args.warmup:
          times['packed'].append(ms_packed)
          times['listed'].append(ms_listed)
        if r < min(args.warmup, 1) + args.loop_rounds:
          _, ms_loop = timed(lambda: loop_coverage(g, cameras, config, masks))
          if r >= min(args.warmup, 1):
            times['loop'].append(ms_loop)
      med = {k: statistics.median(v) for k, v in times.items()}
      print(f"  masks {'on ' if masks else 'off'}  kernel, packed  {summary(times['packed'])}  "
            f"{n * views / med['packed'] / 1e6:7.1f} G pairs/s")
      print(f"             kernel, list    {summary(times['listed'])}")
      print(f"             loop            {summary(times['loop'])}")
      print(f"             loop / kernel: packed {med['loop'] / med['packed']:.1f}x, list {med['loop'] / med['listed']:.1f}x")


if __name__ == '__main__':
  main()
