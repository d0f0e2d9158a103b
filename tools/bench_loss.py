#!/usr/bin/env python
"""Photometric loss (1 - w) L1 + w (1 - SSIM): the fused kernels (csrc/loss.hip) against the torch composition a user
writes without them, same process, same box, same data.

The torch composition is written out below: permute the (H, W, 3) render to NCHW, five grouped 11 x 11 conv2d, the
element-wise SSIM expression, means, and the autograd chain back through all of it.  Both produce the loss and
dL/dimage in (H, W, C); their results are compared first.

Per size (2048^2 x 3 and 4096^2 x 3), forward and forward + backward: events on the stream, warm-up, clocks spun up by
the warm-up rounds, the two variants alternating inside every round, median / min / max over the rounds.  Achieved
GB/s is on the algorithmic traffic of a fused implementation, per image element: the forward reads 2 images and writes
3 partial maps (20 B), the backward reads 3 maps and 2 images and writes the gradient (24 B) = 44 B per element,
0.55 GB at 2048^2 x 3.  The forward timed alone runs without a gradient and writes no maps: 8 B per element.  A device-to-device copy of the same size is timed next to it as the box's stream rate.

    python tools/bench_loss.py [--sizes 2048 4096] [--rounds 20] [--warmup 5]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from taichi_splatting_amd import l1_ssim_loss    # noqa: E402

FRAME_MS = 3.07          # config D render + backward on this machine class (profiles/README.md)
BYTES_FWD, BYTES_BWD = 20, 24
BYTES_FWD_ONLY = 8      # two images read: without a gradient the forward writes no partial maps


def window(device):
  k = torch.arange(11, dtype=torch.float64) - 5
  g = torch.exp(-k * k / (2 * 1.5 * 1.5))
  g = (g / g.sum()).float()
  return torch.outer(g, g).to(device)


def torch_loss(image, target, win, weight=0.2):
  c = image.shape[2]
  k = win.expand(c, 1, 11, 11).contiguous()
  x, y = image.permute(2, 0, 1).unsqueeze(0), target.permute(2, 0, 1).unsqueeze(0)
  mu1, mu2 = F.conv2d(x, k, padding=5, groups=c), F.conv2d(y, k, padding=5, groups=c)
  s11 = F.conv2d(x * x, k, padding=5, groups=c) - mu1 * mu1
  s22 = F.conv2d(y * y, k, padding=5, groups=c) - mu2 * mu2
  s12 = F.conv2d(x * y, k, padding=5, groups=c) - mu1 * mu2
  c1, c2 = 0.01 ** 2, 0.03 ** 2
  ssim = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))).mean()
  return (1 - weight) * (image - target).abs().mean() + weight * (1 - ssim)


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
  target = torch.rand((size, size, 3), device=device, generator=gen)
  image = (target + 0.1 * torch.randn((size, size, 3), device=device, generator=gen)).clamp(0, 1).requires_grad_(True)
  win = window(device)
  elements = image.numel()
  print(f"== {size} x {size} x 3 ({elements * 4 / 1e6:.0f} MB per image)")

  def fwd(loss_fn):
    with torch.no_grad():
      return loss_fn()

  def fwd_bwd(loss_fn):
    image.grad = None
    loss_fn().backward()

  fused = lambda: l1_ssim_loss(image, target)          # noqa: E731
  composed = lambda: torch_loss(image, target, win)    # noqa: E731

  fwd_bwd(fused)
  loss_f, grad_f = fused().detach(), image.grad.clone()
  fwd_bwd(composed)
  loss_t, grad_t = composed().detach(), image.grad.clone()
  print(f"loss fused {float(loss_f):.7f}  torch {float(loss_t):.7f}; gradient: largest {float(grad_t.abs().max()):.3e}, "
        f"largest difference {float((grad_f - grad_t).abs().max()):.3e}")
  assert abs(float(loss_f) - float(loss_t)) < 1e-4 and float((grad_f - grad_t).abs().max()) < 1e-3 * float(grad_t.abs().max())
  del grad_f, grad_t

  src = torch.empty((elements * (BYTES_FWD + BYTES_BWD) // 8,), dtype=torch.float32, device=device)
  dst = torch.empty_like(src)
  variants = {
    'fused fwd': lambda: fwd(fused), 'torch fwd': lambda: fwd(composed),
    'fused fwd+bwd': lambda: fwd_bwd(fused), 'torch fwd+bwd': lambda: fwd_bwd(composed),
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
  total = elements * (BYTES_FWD + BYTES_BWD)
  print(f"fused fwd (no gradient, no maps written): {elements * BYTES_FWD_ONLY / 1e9:.3f} GB in {med['fused fwd']:.3f} ms = "
        f"{elements * BYTES_FWD_ONLY / med['fused fwd'] / 1e6:.0f} GB/s")
  print(f"fused fwd+bwd:  {total / 1e9:.3f} GB in {med['fused fwd+bwd']:.3f} ms = {total / med['fused fwd+bwd'] / 1e6:.0f} GB/s; "
        f"copy of the same bytes (half read, half written): {total / med['copy (same bytes)'] / 1e6:.0f} GB/s")
  print(f"torch / fused: fwd {med['torch fwd'] / med['fused fwd']:.2f}x, fwd+bwd {med['torch fwd+bwd'] / med['fused fwd+bwd']:.2f}x; "
        f"fused fwd+bwd = {100 * med['fused fwd+bwd'] / FRAME_MS:.1f} % of the {FRAME_MS} ms config-D frame")
  return med['torch fwd'] / med['fused fwd'], med['torch fwd+bwd'] / med['fused fwd+bwd']


def main():
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--sizes', type=int, nargs='+', default=[2048, 4096])
  p.add_argument('--rounds', type=int, default=20)
  p.add_argument('--warmup', type=int, default=5)
  args = p.parse_args()
  if not torch.cuda.is_available():
    sys.exit("bench_loss: no GPU visible (there is no CPU fallback to time)")
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
