#!/usr/bin/env python
"""Bilateral-grid slice: the fused kernels (csrc/bilagrid.hip) against the torch composition a user writes without them,
same process, same box, same data.

The torch composition is written out below: luminance, the 5-D grid_sample (bilinear, border, align_corners) of the
(12, L, Gy, Gx) grid at (x, y, luminance), the per-pixel 3 x 4 affine, and the autograd chain back through all of it
(whose grid gradient is a scatter with float atomics).  Both produce the corrected image, dL/dimage and dL/dgrid; their
results are compared first.

Per size (2048^2 x 3 and 4096^2 x 3, grid 16 x 16 x 8), forward and forward + backward: events on the stream, warm-up,
the variants alternating inside every round, median / min / max over the rounds.  Achieved GB/s is on the algorithmic
traffic per pixel in float32: the forward reads and writes one image (24 B), the image gradient reads the image and
the upstream gradient and writes one (36 B), the grid gradient reads the image and the upstream gradient (24 B); the
grid itself is kilobytes.  A device-to-device copy of the same bytes is timed next to it as the box's stream rate.

    python tools/bench_bilagrid.py [--sizes 2048 4096] [--rounds 20] [--warmup 5]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from taichi_splatting_amd import apply_bilateral_grid    # noqa: E402

BYTES_FWD, BYTES_IMAGE_GRAD, BYTES_GRID_GRAD = 24, 36, 24
GRID = (8, 16, 16)       # L, Gy, Gx


def torch_slice(image, grid):
  h, w, _ = image.shape
  u = (torch.arange(w, dtype=image.dtype, device=image.device) + 0.5) / w
  v = (torch.arange(h, dtype=image.dtype, device=image.device) + 0.5) / h
  lum = (image * image.new_tensor([0.299, 0.587, 0.114])).sum(-1).clamp(0, 1)
  coords = torch.stack([(2 * u - 1).expand(h, w), (2 * v - 1)[:, None].expand(h, w), 2 * lum - 1], -1)
  planes = F.grid_sample(grid[None], coords[None, None], mode='bilinear', padding_mode='border', align_corners=True)
  a = planes[0, :, 0].permute(1, 2, 0).reshape(h, w, 3, 4)
  return (a[..., :3] * image[..., None, :]).sum(-1) + a[..., 3]


def event_ms(fn):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end)


def summary(xs):
  return f"median {statistics.median(xs):8.3f} ms  min {min(xs):8.3f}  max {max(xs):8.3f}"


def run(size, rounds, warmup, device):
  gen = torch.Generator(device=device).manual_seed(size)
  image = (torch.rand((size, size, 3), device=device, generator=gen) * 1.2 - 0.1).requires_grad_(True)
  eye = torch.eye(3, 4, device=device).reshape(12, 1, 1, 1)
  grid = (eye + 0.1 * torch.randn((12,) + GRID, device=device, generator=gen)).requires_grad_(True)
  grad_out = torch.randn((size, size, 3), device=device, generator=gen) / (size * size)
  pixels = size * size
  print(f"== {size} x {size} x 3 ({pixels * 12 / 1e6:.0f} MB per image), grid {GRID[2]} x {GRID[1]} x {GRID[0]}")

  def fwd(slice_fn):
    with torch.no_grad():
      return slice_fn(image, grid)

  def fwd_bwd(slice_fn):
    image.grad = grid.grad = None
    slice_fn(image, grid).backward(grad_out)

  results = {}
  for name, fn in (('fused', apply_bilateral_grid), ('torch', torch_slice)):
    fwd_bwd(fn)
    results[name] = (fwd(fn), image.grad.clone(), grid.grad.clone())
  (out_f, gi_f, gg_f), (out_t, gi_t, gg_t) = results['fused'], results['torch']
  # the guide term of dL/dimage jumps where the luminance crosses a bin: two float32 evaluations may land on either side
  # of a crossing for a handful of pixels, so that gradient is compared by the share of pixels that agree
  agree = float(((gi_f - gi_t).abs().amax(-1) <= 1e-3 * gi_t.abs().max()).float().mean())
  print(f"out: largest {float(out_t.abs().max()):.3f}, largest difference {float((out_f - out_t).abs().max()):.3e}; "
        f"dL/dgrid: largest {float(gg_t.abs().max()):.3e}, largest difference {float((gg_f - gg_t).abs().max()):.3e}; "
        f"dL/dimage: {100 * agree:.4f} % of the pixels within 1e-3 of the largest")
  assert float((out_f - out_t).abs().max()) < 1e-4 * float(out_t.abs().max())
  assert float((gg_f - gg_t).abs().max()) < 1e-3 * float(gg_t.abs().max())
  assert agree > 0.999
  del results, out_f, gi_f, gg_f, out_t, gi_t, gg_t

  total = pixels * (BYTES_FWD + BYTES_IMAGE_GRAD + BYTES_GRID_GRAD)
  src = torch.empty((total // 8,), dtype=torch.float32, device=device)
  dst = torch.empty_like(src)
  variants = {
    'fused fwd': lambda: fwd(apply_bilateral_grid), 'torch fwd': lambda: fwd(torch_slice),
    'fused fwd+bwd': lambda: fwd_bwd(apply_bilateral_grid), 'torch fwd+bwd': lambda: fwd_bwd(torch_slice),
    'copy (same bytes)': lambda: dst.copy_(src),
  }
  times = {k: [] for k in variants}
  for r in range(warmup + rounds):
    for name, fn in variants.items():
      ms = event_ms(fn)
      if r >= warmup:
        times[name].append(ms)
  for name, xs in times.items():
    print(f"{name:18s} {summary(xs)}")
  med = {k: statistics.median(v) for k, v in times.items()}
  print(f"fused fwd:      {pixels * BYTES_FWD / 1e9:.3f} GB in {med['fused fwd']:.3f} ms = "
        f"{pixels * BYTES_FWD / med['fused fwd'] / 1e6:.0f} GB/s")
  print(f"fused fwd+bwd:  {total / 1e9:.3f} GB in {med['fused fwd+bwd']:.3f} ms = {total / med['fused fwd+bwd'] / 1e6:.0f} GB/s; "
        f"copy of the same bytes (half read, half written): {total / med['copy (same bytes)'] / 1e6:.0f} GB/s")
  print(f"torch / fused: fwd {med['torch fwd'] / med['fused fwd']:.2f}x, fwd+bwd {med['torch fwd+bwd'] / med['fused fwd+bwd']:.2f}x")
  return med['torch fwd'] / med['fused fwd'], med['torch fwd+bwd'] / med['fused fwd+bwd']


def main():
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--sizes', type=int, nargs='+', default=[2048, 4096])
  p.add_argument('--rounds', type=int, default=20)
  p.add_argument('--warmup', type=int, default=5)
  args = p.parse_args()
  if not torch.cuda.is_available():
    sys.exit("bench_bilagrid: no GPU visible (there is no CPU fallback to time)")
  device = torch.device('cuda:0')
  print(f"{torch.cuda.get_device_name(device)}; torch {torch.__version__}")
  slower = []
  for size in args.sizes:
    ratios = run(size, args.rounds, args.warmup, device)
    if min(ratios) < 1.0:
      slower.append(size)
  if slower:
    print(f"FUSED PATH SLOWER THAN THE TORCH COMPOSITION at {slower}")
    sys.exit(1)


if __name__ == '__main__':
  main()
