#!/usr/bin/env python
"""Wide-feature rasteriser: rasterize_wide (csrc/raster_wide.hip, one pass, contractions on the f32-input MFMA) against
rasterize_with_tiles (the chunked path: ceil(F / 4) passes of the generic kernels), same process, same box, same
tile lists.

One seeded random_2d_gaussians scene (default 1 M splats at 1024 x 1024, tile 16), one tile-list build.  For every width
F: forward, forward + backward with both gradients, forward + backward with the feature gradient only.  Results of the
two paths are compared first.  Timing: device events around each call, warm-up rounds first, the variants alternating
inside every round, median / min / max over the rounds.  Caches are WARM: every call re-reads the same scene, lists
and features (the lists and the 28-byte geometry rows are 35 MB; the F = 128 images are 512 MB each and do not stay).

Achieved rate of the wide forward: 2 * hits * 64 * F_padded FLOP over its median time, against the 155 TFLOP/s the
f32-input MFMA sustains (MI355X, measured figure of the matrix-core tables).  ``hits`` are the (8 x 8 patch, splat)
pairs the kernels' cull test lets through, recounted here in torch with the same arithmetic; F_padded = 32 ceil(F / 32).
It is a whole-call rate (staging, alpha chain and stores included), not a share of the kernel's bound.

    python tools/bench_raster_wide.py [--splats 1000000] [--size 1024] [--widths 8 16 32 64 128] [--rounds 7] [--warmup 2]
"""
import argparse
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from taichi_splatting_amd import RasterConfig, map_to_tiles, rasterize_wide, rasterize_with_tiles    # noqa: E402
from taichi_splatting_amd.misc.renderer2d import project_gaussians2d                                   # noqa: E402
from taichi_splatting_amd.testing import random_2d_gaussians                                           # noqa: E402

MFMA_F32_TFLOPS = 155.0


def event_ms(fn):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end)


def count_patch_hits(points, o2p, ranges, cfg, tiles_wide):
  """(patch, splat) pairs that pass rect_hit of csrc/raster_common.h (the per-wave cull of the raster kernels); the
  tile ranges lie back to back in tile order (checked by the caller), so entry k belongs to the tile it falls into"""
  counts = (ranges[:, 1] - ranges[:, 0]).long()
  tile = torch.repeat_interleave(torch.arange(ranges.shape[0], device=points.device), counts)
  g = points[o2p[:tile.shape[0]].long()]
  mx, my, ax, ay, sx, sy, alpha = g.unbind(1)
  gs = torch.sqrt(2 * torch.log(alpha / cfg.alpha_threshold)) * 1.001
  ex = torch.sqrt((ax * sx * gs) ** 2 + (ay * sy * gs) ** 2) + 0.01
  ey = torch.sqrt((ay * sx * gs) ** 2 + (ax * sy * gs) ** 2) + 0.01
  A, B, C, D = ax / sx / gs, ay / sx / gs, -ay / sy / gs, ax / sy / gs
  hits = 0
  for wx, wy in ((0, 0), (1, 0), (0, 1), (1, 1)):
    dx = (tile % tiles_wide) * 16 + wx * 8 + 4.0 - mx
    dy = (tile // tiles_wide) * 16 + wy * 8 + 4.0 - my
    hit = (dx.abs() <= ex + 3.5) & (dy.abs() <= ey + 3.5)
    hit &= ((A * dx + B * dy).abs() - (A.abs() + B.abs()) * 3.5 <= 1.002)
    hit &= ((C * dx + D * dy).abs() - (C.abs() + D.abs()) * 3.5 <= 1.002)
    hits += int(hit.sum())
  return hits


def main():
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--splats', type=int, default=1000000)
  p.add_argument('--size', type=int, default=1024)
  p.add_argument('--widths', type=int, nargs='+', default=[8, 16, 32, 64, 128])
  p.add_argument('--rounds', type=int, default=7)
  p.add_argument('--warmup', type=int, default=2)
  args = p.parse_args()
  if not torch.cuda.is_available():
    sys.exit("bench_raster_wide: no GPU visible (there is no CPU fallback to time)")
  device = torch.device('cuda:0')
  print(f"{torch.cuda.get_device_name(device)}; torch {torch.__version__}")

  size = (args.size, args.size)
  cfg = RasterConfig(tile_size=16)
  torch.manual_seed(0)
  g = random_2d_gaussians(args.splats, size).to(device)
  points = project_gaussians2d(g).contiguous()
  o2p, ranges = map_to_tiles(points, g.depths, size, cfg)
  ranges = ranges.view(-1, 2)
  tiles_wide = (size[0] + 15) // 16
  runs = (ranges[:, 1] - ranges[:, 0])
  overlaps = int(runs.sum())
  assert int(ranges[0, 0]) == 0 and bool((ranges[1:, 0] == ranges[:-1, 1]).all()), "tile ranges are expected back to back"
  hits = count_patch_hits(points, o2p, ranges, cfg, tiles_wide)
  print(f"scene: {points.shape[0]} splats, {size[0]} x {size[1]}, tile 16: {overlaps} tile overlaps "
        f"(runs {int(runs.min())}..{int(runs.max())}, mean {overlaps / ranges.shape[0]:.1f}), {hits} (patch, splat) hits")
  print(f"timing: device events, {args.warmup} warm-up + {args.rounds} timed rounds, variants alternate inside a round, "
        "caches warm; ms as median [min .. max]")

  verdict = {}
  for f in args.widths:
    gen = torch.Generator(device=device).manual_seed(f)
    feats = torch.rand((points.shape[0], f), device=device, generator=gen)
    grad_out = torch.randn((size[1], size[0], f), device=device, generator=gen)
    ops = {'wide': rasterize_wide, 'chunked': rasterize_with_tiles}

    def forward(op):
      with torch.no_grad():
        return op(points, feats, o2p, ranges, size, cfg).image

    def forward_backward(op, geometry):
      pg, fg = points.detach().requires_grad_(geometry), feats.detach().requires_grad_(True)
      op(pg, fg, o2p, ranges, size, cfg).image.backward(grad_out)
      return pg.grad, fg.grad

    # the two paths compute the same thing (different summation orders, float atomics)
    img_w, img_c = forward(rasterize_wide), forward(rasterize_with_tiles)
    (gp_w, gf_w), (gp_c, gf_c) = forward_backward(rasterize_wide, True), forward_backward(rasterize_with_tiles, True)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    print(f"== F = {f}: image max difference {float((img_w - img_c).abs().max()):.2e}; gradients, of the largest entry: "
          f"d gaussians2d {rel(gp_w, gp_c):.2e}, d features {rel(gf_w, gf_c):.2e}")
    del img_w, img_c, gp_w, gf_w, gp_c, gf_c

    variants = {}
    for name, op in ops.items():
      variants[f'{name} fwd'] = lambda op=op: forward(op)
      variants[f'{name} fwd+bwd (both)'] = lambda op=op: forward_backward(op, True)
      variants[f'{name} fwd+bwd (features)'] = lambda op=op: forward_backward(op, False)
    times = {k: [] for k in variants}
    for r in range(args.warmup + args.rounds):
      for name, fn in variants.items():
        ms = event_ms(fn)
        if r >= args.warmup:
          times[name].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    for kind in ('fwd', 'fwd+bwd (both)', 'fwd+bwd (features)'):
      w, c = times[f'wide {kind}'], times[f'chunked {kind}']
      print(f"  {kind:20s} wide {med[f'wide {kind}']:9.3f} [{min(w):9.3f} .. {max(w):9.3f}]   "
            f"chunked {med[f'chunked {kind}']:9.3f} [{min(c):9.3f} .. {max(c):9.3f}]   "
            f"chunked / wide {med[f'chunked {kind}'] / med[f'wide {kind}']:6.2f}x")
    flop = 2.0 * hits * 64 * 32 * math.ceil(f / 32)
    rate = flop / (med['wide fwd'] * 1e-3) / 1e12
    print(f"  wide fwd: {flop / 1e9:.1f} GFLOP on the matrix cores in {med['wide fwd']:.3f} ms = {rate:.2f} TFLOP/s "
          f"= {100 * rate / MFMA_F32_TFLOPS:.1f} % of {MFMA_F32_TFLOPS:.0f} TFLOP/s (whole call)")
    w, c = times['wide fwd+bwd (both)'], times['chunked fwd+bwd (both)']
    verdict[f] = max(w) < min(c)          # faster by more than the spread: the slowest wide round beats the fastest chunked one
  print("fwd+bwd (both), wide faster than chunked beyond the spread of the rounds: "
        + ", ".join(f"F = {f}: {'yes' if v else 'NO'}" for f, v in verdict.items()))
  if not all(verdict.get(f, True) for f in (32, 64)):
    print("ACCEPTANCE MISSED: the wide path must win at F = 32 and F = 64")
    sys.exit(1)


if __name__ == '__main__':
  main()
