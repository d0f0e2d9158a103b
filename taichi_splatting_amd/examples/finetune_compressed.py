"""Fine-tune a vector-quantised scene without decoding it (the codebook tuning step of Compact3D and of Niedermayr et
al., which ``scene_codec.py`` follows; the reference package has no counterpart).

A random degree-3 scene is compressed to a few SH codes (``compress_scene``), target images are rendered from the
original, and ``dc`` and ``sh_codebook`` are tuned with ``torch.optim.Adam`` through ``render_compressed``: the colours
come from the stored form (csrc/sh_coded.hip), the codebook gradient is summed per code in a fixed order, and neither
the decoded (N, 3, 16) feature tensor nor its gradient ever exists.  The indices stay as assigned.

  python -m taichi_splatting_amd.examples.finetune_compressed --n 2000 --codes 8 --cameras 2 --steps 50 --lr 1e-3

Prints progress to stderr and ONE JSON line: the mean squared error over the cameras and its PSNR before and after.
"""
from __future__ import annotations

import argparse
import json
import math
import sys

import torch

from ..data_types import RasterConfig
from ..perspective import CameraParams
from ..renderer import render_gaussians
from ..scene_codec import compress_scene, render_compressed
from ..testing import random_3d_gaussians, random_camera


def shifted_cameras(camera: CameraParams, count: int):
  """``count`` cameras: the given one and copies moved sideways by multiples of 0.15 (camera x axis), so that every
  gaussian is seen from slightly different directions"""
  cameras = []
  for v in range(count):
    T = camera.T_camera_world.clone()
    T[0, 3] += 0.15 * v
    cameras.append(CameraParams(T_camera_world=T, projection=camera.projection, image_size=camera.image_size,
                                near_plane=camera.near_plane, far_plane=camera.far_plane))
  return cameras


def mean_loss(scene, cameras, targets, config) -> float:
  with torch.no_grad():
    losses = [torch.nn.functional.mse_loss(render_compressed(scene, cam, config).image, target)
              for cam, target in zip(cameras, targets)]
  return float(torch.stack(losses).mean())


def psnr(mse: float) -> float:
  return -10.0 * math.log10(mse) if mse > 0 else float('inf')


def main(argv=None):
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--n', type=int, default=20000)
  p.add_argument('--codes', type=int, default=64)
  p.add_argument('--cameras', type=int, default=4)
  p.add_argument('--steps', type=int, default=200)
  p.add_argument('--lr', type=float, default=1e-3)
  p.add_argument('--size', type=int, nargs=2, default=(320, 192), metavar=('W', 'H'))
  p.add_argument('--seed', type=int, default=0)
  args = p.parse_args(argv)
  if not torch.cuda.is_available():
    sys.exit("finetune_compressed: no GPU visible (the renderer has no CPU fallback)")
  device = torch.device('cuda:0')
  torch.manual_seed(args.seed)
  camera = random_camera(image_size=tuple(args.size))
  original = random_3d_gaussians(args.n, camera)
  original = original.replace(feature=(torch.rand(args.n, 3, 16) - 0.5) * 0.8).to(device)
  cameras = [cam.to(device=device) for cam in shifted_cameras(camera, args.cameras)]
  config = RasterConfig()

  with torch.no_grad():
    targets = [render_gaussians(original, cam, config, use_sh=True).image for cam in cameras]
  scene = compress_scene(original, sh_codes=args.codes, iterations=10, seed=args.seed)
  scene.dc.requires_grad_(True)
  scene.sh_codebook.requires_grad_(True)
  optimiser = torch.optim.Adam([scene.dc, scene.sh_codebook], lr=args.lr)

  initial = mean_loss(scene, cameras, targets, config)
  print(f"{args.n} gaussians, {args.codes} codes, {args.cameras} cameras: MSE {initial:.6f} ({psnr(initial):.2f} dB) before",
        file=sys.stderr, flush=True)
  for step in range(args.steps):
    optimiser.zero_grad(set_to_none=True)
    for cam, target in zip(cameras, targets):
      loss = torch.nn.functional.mse_loss(render_compressed(scene, cam, config).image, target) / len(cameras)
      loss.backward()
    optimiser.step()
    if (step + 1) % 25 == 0:
      print(f"step {step + 1}: MSE {mean_loss(scene, cameras, targets, config):.6f}", file=sys.stderr, flush=True)
  final = mean_loss(scene, cameras, targets, config)
  print(f"MSE {final:.6f} ({psnr(final):.2f} dB) after {args.steps} steps", file=sys.stderr, flush=True)
  print(json.dumps(dict(n=args.n, codes=args.codes, cameras=args.cameras, steps=args.steps, lr=args.lr,
                        initial_loss=initial, final_loss=final, psnr_before_db=round(psnr(initial), 3),
                        psnr_after_db=round(psnr(final), 3))), flush=True)


if __name__ == '__main__':
  main()
