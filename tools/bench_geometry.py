#!/usr/bin/env python
"""Geometry: the fused kernels (csrc/geometry.hip) against the torch composition a user writes without them — the
formulas of tests/geometry_oracle.py in float32 on the GPU with autograd — same process, same box, same data.

  normals      gaussian_normals forward + backward at N rows (default 6 M) against the composition
  consistency  normal_consistency forward + backward at 1024^2 and 2048^2 (F = 5) against the composition
  frame        render_geometry (F = 5) + its backward beside the colour frame of the bench scene it rides on
               (bench.py's scene: N gaussians, SH degree 3, 2048^2, tile 16): colour alone, and colour + geometry

Events on the stream, warm-up, the variants alternating inside every round, median / min / max over the rounds; a fused
pair counts as faster only when its slowest round beats the composition's fastest.  Results are compared first.
Achieved GB/s is on the algorithmic float32 traffic: normals forward 40 B read + 13 written per row, backward 29 + 16;
consistency forward 5 channels read (20 B per pixel), backward 20 read + 20 written.

    python tools/bench_geometry.py [--rows 6000000] [--sizes 1024 2048] [--frame-n 6000000] [--rounds 20] [--warmup 5]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from taichi_splatting_amd import (Gaussians3D, RasterConfig, gaussian_normals, normal_consistency,     # noqa: E402
                                  render_gaussians, render_geometry)
from tests import geometry_oracle as go                                                                # noqa: E402

NORMAL_BYTES = 40 + 13 + 29 + 16
CONSISTENCY_BYTES = 20 + 20 + 20


def event_ms(fn):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end)


def summary(xs):
  return f"median {statistics.median(xs):8.3f} ms  min {min(xs):8.3f}  max {max(xs):8.3f}"


def interleaved(variants, rounds, warmup):
  times = {k: [] for k in variants}
  for r in range(warmup + rounds):
    for name, fn in variants.items():
      ms = event_ms(fn)
      if r >= warmup:
        times[name].append(ms)
  for name, xs in times.items():
    print(f"{name:28s} {summary(xs)}")
  return times


def verdict(times, fused, torch_name):
  f, t = times[fused], times[torch_name]
  ratio = statistics.median(t) / statistics.median(f)
  outside = max(f) < min(t)
  print(f"torch / fused: {ratio:.2f}x; the fused pair's slowest round {'beats' if outside else 'DOES NOT beat'} "
        f"the composition's fastest ({max(f):.3f} against {min(t):.3f} ms)")
  return outside


def bench_normals(n, rounds, warmup, device):
  gen = torch.Generator(device=device).manual_seed(n)
  rand = lambda *shape: torch.randn(shape, device=device, generator=gen)
  position, log_scaling, rotation = rand(n, 3) * 2, rand(n, 3) * 0.7 - 2, rand(n, 4).requires_grad_(True)
  centre = torch.tensor([0.3, -0.2, -6.0], device=device)
  grad_out = rand(n, 3)
  scene = Gaussians3D(position=position, log_scaling=log_scaling, rotation=rotation,
                      alpha_logit=torch.zeros((n, 1), device=device), feature=torch.zeros((n, 3), device=device), batch_size=(n,))
  print(f"== gaussian_normals, {n} rows, forward + backward")

  def fused():
    rotation.grad = None
    gaussian_normals(scene, centre).backward(grad_out)

  def composed():
    rotation.grad = None
    go.normals(position, log_scaling, rotation, centre).backward(grad_out)

  fused()
  out_f, grad_f = gaussian_normals(scene, centre).detach(), rotation.grad.clone()
  composed()
  out_t, grad_t = go.normals(position, log_scaling, rotation, centre).detach(), rotation.grad.clone()
  same = (out_f - out_t).abs().amax(1) < 1e-5          # a row whose n . (p - c) is a rounding from 0 may take either sign
  print(f"rows that agree to 1e-5: {100 * float(same.float().mean()):.5f} %; rotation gradient on them: largest "
        f"{float(grad_t[same].abs().max()):.3e}, largest difference {float((grad_f - grad_t)[same].abs().max()):.3e}")
  assert float(same.float().mean()) > 0.9999
  assert float((grad_f - grad_t)[same].abs().max()) < 1e-4 * float(grad_t[same].abs().max())
  del out_f, out_t, grad_f, grad_t, same
  src = torch.empty((n * NORMAL_BYTES // 8,), dtype=torch.float32, device=device)
  dst = torch.empty_like(src)
  times = interleaved({'fused fwd+bwd': fused, 'torch fwd+bwd': composed, 'copy (same bytes)': lambda: dst.copy_(src)},
                      rounds, warmup)
  med = statistics.median(times['fused fwd+bwd'])
  print(f"fused: {n * NORMAL_BYTES / 1e9:.3f} GB in {med:.3f} ms = {n * NORMAL_BYTES / med / 1e6:.0f} GB/s; copy of the same "
        f"bytes: {n * NORMAL_BYTES / statistics.median(times['copy (same bytes)']) / 1e6:.0f} GB/s")
  return verdict(times, 'fused fwd+bwd', 'torch fwd+bwd')


def bench_consistency(size, rounds, warmup, device):
  accum, proj, _ = go.make_image(size, size)
  accum, proj = accum.float().to(device).requires_grad_(True), proj.float().to(device)
  pixels = size * size
  print(f"== normal_consistency, {size} x {size} x 5, forward + backward")

  def fused():
    accum.grad = None
    normal_consistency(accum, 0, 1, 2, proj).backward()

  def composed():
    accum.grad = None
    go.consistency(accum, 0, 1, 2, proj)[0].backward()

  fused()
  loss_f, grad_f = float(normal_consistency(accum, 0, 1, 2, proj).detach()), accum.grad.clone()
  composed()
  loss_t, grad_t = float(go.consistency(accum, 0, 1, 2, proj)[0].detach()), accum.grad.clone()
  close = float(((grad_f - grad_t).abs() <= 1e-3 * grad_t.abs().max()).float().mean())
  print(f"loss {loss_f:.7f} (fused) {loss_t:.7f} (torch); gradient: largest {float(grad_t.abs().max()):.3e}, "
        f"{100 * close:.4f} % of the entries within 1e-3 of it")
  assert abs(loss_f - loss_t) < 1e-4 * abs(loss_t) and close > 0.999
  del grad_f, grad_t
  src = torch.empty((pixels * CONSISTENCY_BYTES // 8,), dtype=torch.float32, device=device)
  dst = torch.empty_like(src)
  times = interleaved({'fused fwd+bwd': fused, 'torch fwd+bwd': composed, 'copy (same bytes)': lambda: dst.copy_(src)},
                      rounds, warmup)
  med = statistics.median(times['fused fwd+bwd'])
  print(f"fused: {pixels * CONSISTENCY_BYTES / 1e9:.3f} GB in {med:.3f} ms = {pixels * CONSISTENCY_BYTES / med / 1e6:.0f} GB/s; "
        f"copy of the same bytes: {pixels * CONSISTENCY_BYTES / statistics.median(times['copy (same bytes)']) / 1e6:.0f} GB/s")
  return verdict(times, 'fused fwd+bwd', 'torch fwd+bwd')


def bench_frame(n, size, rounds, warmup, device):
  from taichi_splatting_amd.testing import random_camera, random_3d_gaussians
  torch.manual_seed(0)
  cam = random_camera(image_size=(size, size))
  g = random_3d_gaussians(n, cam, scale_factor=1.0, alpha_range=(0.1, 0.9), margin=0.0)
  g = g.replace(feature=(torch.rand(n, 3, 16) - 0.5) * 0.5).to(device).requires_grad_(True)
  cam = cam.to(device=device)
  config = RasterConfig(tile_size=16)
  weights = torch.rand((size, size, 3), device=device)
  print(f"== render_geometry (F = 5) beside the colour frame: {n} gaussians, SH degree 3, {size} x {size}, forward + backward")

  def zero():
    for t in (g.position, g.log_scaling, g.rotation, g.alpha_logit, g.feature):
      t.grad = None

  def colour():
    zero()
    (render_gaussians(g, cam, config, use_sh=True).image * weights).sum().backward()

  def colour_geometry():
    zero()
    r = render_gaussians(g, cam, config, use_sh=True)
    geo = render_geometry(r, g)
    ((r.image * weights).sum() + normal_consistency(geo.accum, 0, 1, 2, cam.projection) + geo.depth.mean()).backward()

  times = interleaved({'colour frame': colour, 'colour + geometry + losses': colour_geometry}, rounds, warmup)
  a, b = statistics.median(times['colour frame']), statistics.median(times['colour + geometry + losses'])
  print(f"the F = 5 geometry pass, its two losses and their backward add {b - a:.3f} ms to a {a:.3f} ms colour step ({b / a:.2f}x)")


def main():
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--rows', type=int, default=6_000_000)
  p.add_argument('--sizes', type=int, nargs='*', default=[1024, 2048])
  p.add_argument('--frame-n', type=int, default=6_000_000, help='0 skips the frame measurement')
  p.add_argument('--frame-size', type=int, default=2048)
  p.add_argument('--rounds', type=int, default=20)
  p.add_argument('--warmup', type=int, default=5)
  args = p.parse_args()
  if not torch.cuda.is_available():
    sys.exit("bench_geometry: no GPU visible (there is no CPU fallback to time)")
  device = torch.device('cuda:0')
  print(f"{torch.cuda.get_device_name(device)}; torch {torch.__version__}")
  slower = []
  if args.rows and not bench_normals(args.rows, args.rounds, args.warmup, device):
    slower.append('normals')
  for size in args.sizes:
    if not bench_consistency(size, args.rounds, args.warmup, device):
      slower.append(f'consistency {size}')
  if args.frame_n:
    bench_frame(args.frame_n, args.frame_size, max(args.rounds // 2, 3), 2, device)
  if slower:
    print(f"FUSED PATH NOT FASTER THAN THE TORCH COMPOSITION OUTSIDE THE SPREAD: {slower}")
    sys.exit(1)


if __name__ == '__main__':
  main()
