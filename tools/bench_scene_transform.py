#!/usr/bin/env python
"""Gaussians3D.transformed (csrc/scene_transform.hip) against the torch composition it replaces, same process, same box.

Scene: N gaussians, SH degree 3, float32 (6 M: the 1.15 GB feature tensor load_ply produces).  Four variants,
alternating inside every round after warm-up, device time from events around the call:

    launch, in place       ms_scene_transform alone on a transform packed beforehand (what a captured graph replays)
    kernel, in place       g.transformed(m, inplace=True) under no_grad: the same launch behind the host's validation
                           of m and its SH matrices (about 2 ms of Python, during which the device waits)
    kernel, out of place   g.transformed(m)                      (allocates the four outputs)
    torch chain            scaled + transform_rigid's geometry (quaternion product instead of the matrix round trip) and
                           one band-sliced matmul per SH band, concatenated

The results are compared first (float32, the test suite's bounds).  Bytes moved = every field read once and written
once, divided by the time, printed beside the device copy of the same bytes; run tools/ubench_stream.hip in the same
session for what the box streams.  Also shown: the peak-memory growth of one in-place call (must stay below one feature
tensor: no N x 48 temporary).  That the call is ONE launch is a kernel trace's to show:

    rocprofv3 --kernel-trace --stats -- python tools/bench_scene_transform.py --rows 1000000 --trace-calls 5

runs nothing but the set-up and five in-place calls (five scene_transform_kernel dispatches and no other kernel after
the set-up's fills).

    python tools/bench_scene_transform.py [--rows 6000000] [--rounds 10] [--warmup 3]
"""
import argparse
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from taichi_splatting_amd import Gaussians3D, sh_rotation_matrices                   # noqa: E402
from taichi_splatting_amd.data_types import _quat_to_mat                             # noqa: E402
from taichi_splatting_amd.spherical_harmonics import pack_scene_transform, rotation_to_quat, scene_transform   # noqa: E402


def make_scene(n, device):
  g = torch.Generator(device=device).manual_seed(n)
  r = lambda *shape: torch.randn(*shape, device=device, generator=g)
  return Gaussians3D(position=3.0 * r(n, 3), log_scaling=r(n, 3) - 3.0, rotation=r(n, 4), alpha_logit=r(n, 1),
                     feature=0.5 * r(n, 3, 16), batch_size=(n,))


def make_transform():
  q = torch.randn(4, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
  m = torch.eye(4, dtype=torch.float64)
  m[:3, :3] = 1.7 * _quat_to_mat(q / q.norm())
  m[:3, 3] = torch.tensor([6.0, -7.0, 5.0], dtype=torch.float64)
  return m


def torch_chain(g, s, R, t, q_r, bands):
  """the same scene from torch operators: R, t, q_r and the band matrices are device tensors prepared once"""
  position = s * (g.position @ R.T) + t
  log_scaling = g.log_scaling + math.log(s)
  x, y, z, w = g.rotation.unbind(-1)
  ax, ay, az, aw = q_r.unbind(-1)
  rotation = torch.stack([aw * x + ax * w + ay * z - az * y, aw * y - ax * z + ay * w + az * x,
                          aw * z + ax * y - ay * x + az * w, aw * w - ax * x - ay * y - az * z], dim=-1)
  feature = torch.cat([g.feature[:, :, :1]] + [g.feature[:, :, l * l:(l + 1) * (l + 1)] @ bands[l - 1].T for l in (1, 2, 3)], dim=2)
  return g.replace(position=position, log_scaling=log_scaling, rotation=rotation, feature=feature)


def timed(fn):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  out = fn()
  end.record()
  end.synchronize()
  return out, start.elapsed_time(end)


def summary(xs):
  return f"median {statistics.median(xs):8.3f} ms  min {min(xs):8.3f}  max {max(xs):8.3f}"


def main():
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--rows', type=int, default=6_000_000)
  p.add_argument('--rounds', type=int, default=10)
  p.add_argument('--warmup', type=int, default=3)
  p.add_argument('--trace-calls', type=int, default=0, metavar='K', help="only K in-place calls after the set-up (for a kernel trace)")
  args = p.parse_args()
  if not torch.cuda.is_available():
    sys.exit("bench_scene_transform: no GPU visible (there is no CPU fallback to time)")
  device = torch.device('cuda:0')
  n = args.rows
  scene, m = make_scene(n, device), make_transform()
  torch.cuda.synchronize()

  if args.trace_calls:
    with torch.no_grad():
      for _ in range(args.trace_calls):
        scene.transformed(m, inplace=True)
    torch.cuda.synchronize()
    print(f"{args.trace_calls} in-place calls of Gaussians3D.transformed on {n} gaussians")
    return

  print(f"{torch.cuda.get_device_name(device)}; torch {torch.__version__}; N = {n}, SH degree 3, float32")
  s = 1.7
  R64 = m[:3, :3] / s
  R, t = R64.float().to(device), m[:3, 3].float().to(device)
  q_r = rotation_to_quat(R64).float().to(device)
  bands = [b.float().to(device) for b in sh_rotation_matrices(R64, 3)[1:]]

  # the two paths agree (float32 against float32: twice the suite's one-application bounds)
  a, b = scene.transformed(m), torch_chain(scene, s, R, t, q_r, bands)
  worst = {k: float((getattr(a, k) - getattr(b, k)).abs().max()) for k in ('position', 'log_scaling', 'rotation', 'feature')}
  print("largest difference kernel - torch chain: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
  assert worst['position'] < 1e-4 and worst['log_scaling'] < 4e-6 and worst['rotation'] < 1e-5 and worst['feature'] < 2e-5, worst
  del a, b

  # peak memory of one in-place call
  feature_bytes = scene.feature.numel() * scene.feature.element_size()
  work = scene.clone()
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats(device)
  before = torch.cuda.max_memory_allocated(device)
  with torch.no_grad():
    work.transformed(m, inplace=True)
  torch.cuda.synchronize()
  growth = torch.cuda.max_memory_allocated(device) - before
  print(f"in-place call: peak allocated memory grew by {growth} bytes (one feature tensor: {feature_bytes})")
  assert growth < feature_bytes

  moved = 2 * sum(getattr(scene, k).numel() * 4 for k in ('position', 'log_scaling', 'rotation', 'feature'))
  src, dst = torch.empty(moved // 8, device=device), torch.empty(moved // 8, device=device)
  times = dict(launch=[], inplace=[], out=[], torch=[], copy=[])
  packed = pack_scene_transform(s, R64, m[:3, 3], 3)
  fields = lambda g: dict(position=g.position, log_scaling=g.log_scaling, rotation=g.rotation, feature=g.feature)
  for r in range(args.warmup + args.rounds):
    _, ms_launch = timed(lambda: scene_transform(packed, **fields(work), **{'out_' + k: v for k, v in fields(work).items()}))
    with torch.no_grad():
      _, ms_inplace = timed(lambda: work.transformed(m, inplace=True))
    out, ms_out = timed(lambda: scene.transformed(m))
    del out
    out, ms_torch = timed(lambda: torch_chain(scene, s, R, t, q_r, bands))
    del out
    _, ms_copy = timed(lambda: dst.copy_(src))
    if r >= args.warmup:
      for key, ms in (('launch', ms_launch), ('inplace', ms_inplace), ('out', ms_out), ('torch', ms_torch), ('copy', ms_copy)):
        times[key].append(ms)
    if r % 4 == 3:
      work = scene.clone()            # (repeated in-place scaling by 1.7 would overflow after a hundred rounds)
  labels = dict(launch='launch, in place    ', inplace='kernel, in place    ', out='kernel, out of place', torch='torch chain         ', copy='copy (same bytes)   ')
  for key, label in labels.items():
    print(f"{label} {summary(times[key])}")
  med = {k: statistics.median(v) for k, v in times.items()}
  print(f"bytes moved (every field read once, written once): {moved / 1e9:.3f} GB")
  for key in ('launch', 'inplace', 'out', 'copy'):
    print(f"  {labels[key].strip():22s} {moved / med[key] / 1e9:.2f} TB/s")
  print(f"torch chain / kernel: launch alone {med['torch'] / med['launch']:.2f}x, in place {med['torch'] / med['inplace']:.2f}x, "
        f"out of place {med['torch'] / med['out']:.2f}x")


if __name__ == '__main__':
  main()
