"""Fit per-image bilateral grids to photographs that differ in exposure, white balance and tone curve (the appearance
model of "Bilateral guided radiance field processing"; the reference package has no counterpart).

A fixed small 3-D scene is rendered from a few cameras.  The targets are those renders under a different gain, tint and
gamma per view, as photographs of one scene differ.  The scene stays as it is: ``torch.optim.Adam`` on the
``BilateralGrids`` alone drives ``l1_ssim_loss(apply_bilateral_grid(render, grid_i), target_i)`` (plus a small
total-variation term), every image-sized step a fused kernel (csrc/bilagrid.hip, csrc/loss.hip).

The loop stops once the mean photometric loss is at or below ``--tol`` (1e-6: a mean error of a thousandth of a grey
level of an 8-bit photograph, and 16 float32 roundings of the O(1) quantity ``1 - SSIM``): a fit that good has nothing
left to learn, and Adam must not be run on it.  Adam divides a gradient by its own running size, so where the true
gradient vanishes it turns rounding noise into steps of the order of the learning rate: with targets EQUAL to the
renders the identity grids return the render bit for bit and the loss starts at 4e-10, yet without the stop the SSIM
gradient's rounding noise moves the grids, the L1 term answers every departure, however small, with a gradient of full
size, and after 150 steps the grids have wandered 8.6e-3 from the identity (7.7e-3 in float64) and the loss has RISEN to
9e-4 (``--tol 0`` shows it).  With the stop, identical photographs leave the grids exactly where they are.

  python -m taichi_splatting_amd.examples.fit_appearance --size 128 128 --views 3 --steps 150

Prints progress to stderr and ONE JSON line: the mean loss over the views before and after.
"""
from __future__ import annotations

import argparse
import json
import sys

import torch

from ..appearance import BilateralGrids
from ..data_types import RasterConfig
from ..loss import l1_ssim_loss
from ..renderer import render_gaussians
from ..testing import random_3d_gaussians, random_camera
from .finetune_compressed import shifted_cameras

# per view: gain, (r, g, b) tint, gamma
LOOKS = [(0.70, (1.00, 0.95, 0.85), 1.00), (1.25, (0.90, 1.00, 1.10), 0.80), (1.00, (1.10, 0.92, 1.00), 1.25),
         (0.85, (0.95, 1.05, 1.00), 0.90), (1.15, (1.05, 1.00, 0.90), 1.10)]


def photograph(render: torch.Tensor, view: int, identity: bool = False) -> torch.Tensor:
  """the render as view ``view``'s camera would have recorded it"""
  if identity:
    return render.clone()
  gain, tint, gamma = LOOKS[view % len(LOOKS)]
  return (gain * render * render.new_tensor(tint)).clamp(1e-4, 1.0) ** gamma


def mean_loss(grids: BilateralGrids, renders, targets) -> float:
  with torch.no_grad():
    return float(torch.stack([l1_ssim_loss(grids(r, i), t) for i, (r, t) in enumerate(zip(renders, targets))]).mean())


def fit(size=(64, 64), views: int = 3, steps: int = 150, lr: float = 0.01, tv_weight: float = 1.0, n: int = 2000,
        grid_shape=(16, 16, 8), identity_targets: bool = False, seed: int = 0, device='cuda:0',
        dtype: torch.dtype = torch.float32, tol: float = 1e-6, log=None):
  """``dict(initial_loss, final_loss, grids, steps_taken)``: the mean photometric loss over the views before and after at
  most ``steps`` of Adam on the grids, the fitted ``BilateralGrids`` and the steps taken before the loss was at or
  below ``tol`` (one host read of the loss per step: this is the example's stopping rule, not the library's)"""
  device = torch.device(device)
  torch.manual_seed(seed)
  camera = random_camera(image_size=tuple(size))
  scene = random_3d_gaussians(n, camera).to(device)
  cameras = [cam.to(device=device) for cam in shifted_cameras(camera, views)]
  with torch.no_grad():
    renders = [render_gaussians(scene, cam, RasterConfig()).image.clamp(0, 1).to(dtype).contiguous() for cam in cameras]
  targets = [photograph(r, i, identity_targets) for i, r in enumerate(renders)]
  grids = BilateralGrids(views, grid_shape, dtype=dtype, device=device)
  optimiser = torch.optim.Adam(grids.parameters(), lr=lr)
  initial = mean_loss(grids, renders, targets)
  taken = 0
  for step in range(steps):
    optimiser.zero_grad(set_to_none=True)
    photometric = torch.stack([l1_ssim_loss(grids(r, i), t) for i, (r, t) in enumerate(zip(renders, targets))]).mean()
    if float(photometric.detach()) <= tol:       # converged: what is left of the gradient is rounding noise
      break
    (photometric + tv_weight * grids.tv_loss()).backward()
    optimiser.step()
    taken = step + 1
    if log is not None and taken % 25 == 0:
      log(f"step {taken}: loss {mean_loss(grids, renders, targets):.6f}")
  return dict(initial_loss=initial, final_loss=mean_loss(grids, renders, targets), grids=grids, steps_taken=taken)


def main(argv=None):
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--size', type=int, nargs=2, default=(128, 128), metavar=('W', 'H'))
  p.add_argument('--views', type=int, default=3)
  p.add_argument('--steps', type=int, default=150)
  p.add_argument('--lr', type=float, default=0.01)
  p.add_argument('--tv-weight', type=float, default=1.0)
  p.add_argument('--n', type=int, default=2000)
  p.add_argument('--seed', type=int, default=0)
  p.add_argument('--dtype', choices=('float32', 'float64'), default='float32')
  p.add_argument('--tol', type=float, default=1e-6, help="stop once the mean photometric loss is at or below this")
  args = p.parse_args(argv)
  if not torch.cuda.is_available():
    sys.exit("fit_appearance: no GPU visible (the renderer has no CPU fallback)")
  result = fit(tuple(args.size), args.views, args.steps, args.lr, args.tv_weight, args.n, seed=args.seed,
               dtype=getattr(torch, args.dtype), tol=args.tol,
               log=lambda line: print(line, file=sys.stderr, flush=True))
  print(f"loss {result['initial_loss']:.6f} before, {result['final_loss']:.6f} after {result['steps_taken']} steps", file=sys.stderr, flush=True)
  print(json.dumps(dict(size=list(args.size), views=args.views, steps=result['steps_taken'], lr=args.lr,
                        initial_loss=result['initial_loss'], final_loss=result['final_loss'])), flush=True)


if __name__ == '__main__':
  main()
