#!/usr/bin/env python
"""Densification step, torch path against the fused kernels (csrc/densify.hip), same process, same box.

Scene: the benchmark's shape — N rows x 59 floats in the five Gaussians3D tensors (SH degree 3) with VisibilityAwareAdam
state (two moments per parameter, running visibility, total weight) — 5 % of the rows pruned, 5 % split into two.
Both paths produce children that are copies of their parents (the rows and the state are what the step moves; the 3-D
child geometry is one more small kernel, timed separately), and their results are compared bit for bit first.

Per path and size, after warm-up, alternating the two: device time (events on the stream around the step) and wall time
(host clock from the call to a device synchronise: host reads, allocation and the optimiser rebuild included).

    python tools/bench_densify.py [--rows 6000000 100000] [--rounds 7] [--warmup 2]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from taichi_splatting_amd.misc.densify import split_children3d                      # noqa: E402
from taichi_splatting_amd.optim import ParameterClass, VisibilityAwareAdam, plan_densify   # noqa: E402

SHAPES = dict(position=(3,), log_scaling=(3,), rotation=(4,), alpha_logit=(1,), feature=(3, 16))


def make_params(n, device):
  g = torch.Generator(device=device).manual_seed(n)
  tensors = {k: torch.randn((n, *s), device=device, generator=g) for k, s in SHAPES.items()}
  params = ParameterClass(tensors, {k: dict(lr=1e-3) for k in SHAPES}, optimizer=VisibilityAwareAdam)
  for k in SHAPES:
    params.tensors[k].grad = torch.randn((n, *SHAPES[k]), device=device, generator=g)
  params.step(indexes=None, visibility=torch.rand(n, device=device, generator=g) + 0.1)     # creates every state tensor
  params.zero_grad()
  return params


def torch_step(params, prune, split):
  """The chain of examples/fit_image_gaussians.py split_prune with parent copies as children."""
  to_split = params[split] if bool(split.any()) else None
  kept = params[~(split | prune)]
  if to_split is not None:
    kept = kept.append_tensors({k: torch.repeat_interleave(t.detach(), 2, dim=0) for k, t in to_split.tensors.items()})
  return kept


def fused_step(params, prune, split):
  return params.densify(prune, split, 2)


def timed(fn, device):
  torch.cuda.synchronize(device)
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  t0 = time.perf_counter()
  start.record()
  out = fn()
  end.record()
  torch.cuda.synchronize(device)
  wall = (time.perf_counter() - t0) * 1e3
  return out, start.elapsed_time(end), wall


def summary(xs):
  return f"median {statistics.median(xs):8.3f} ms  min {min(xs):8.3f}  max {max(xs):8.3f}"


def bytes_moved(params, plan):
  """Bytes the move kernel has to read and write: parameters (children copy their parent) and state (children zero)."""
  total = 8 * plan.n_out
  for t in params.tensors.values():
    total += (t.numel() // plan.n) * t.element_size() * 2 * plan.n_out
  for st in params.tensor_state.values():
    for t in st.values():
      total += (t.numel() // plan.n) * t.element_size() * (plan.n_kept + plan.n_out)
  return total


def run(n, rounds, warmup, device):
  params = make_params(n, device)
  g = torch.Generator(device=device).manual_seed(1)
  u = torch.rand(n, device=device, generator=g)
  prune, split = u < 0.05, (u >= 0.05) & (u < 0.10)
  state_floats = sum(t.numel() // n for st in params.tensor_state.values() for t in st.values())
  print(f"== {n} rows x {sum(t.numel() // n for t in params.tensors.values())} parameter floats + {state_floats} state floats; "
        f"{int(prune.sum())} pruned, {int(split.sum())} split into 2")

  a, b = torch_step(params, prune, split), fused_step(params, prune, split)
  same = all(torch.equal(a.tensors[k].detach(), b.tensors[k].detach()) for k in SHAPES)
  sa, sb = a.tensor_state, b.tensor_state
  same = same and all(torch.equal(sa[k][s], sb[k][s]) for k in sa for s in sa[k])
  print(f"results equal bit for bit: {same} ({b.batch_size[0]} rows)")
  assert same
  del a, b, sa, sb

  times = dict(torch=([], []), fused=([], []), move=([], []), plan=([], []), split3d=([], []))
  for r in range(warmup + rounds):
    for name, fn in (('torch', torch_step), ('fused', fused_step)):
      out, dev_ms, wall_ms = timed(lambda: fn(params, prune, split), device)
      del out
      if r >= warmup:
        times[name][0].append(dev_ms); times[name][1].append(wall_ms)
    plan, dev_ms, wall_ms = timed(lambda: plan_densify(prune, split, 2), device)
    if r >= warmup:
      times['plan'][0].append(dev_ms); times['plan'][1].append(wall_ms)
    out, dev_ms, wall_ms = timed(lambda: params.densify(prune, split, 2, plan=plan), device)
    if r >= warmup:
      times['move'][0].append(dev_ms); times['move'][1].append(wall_ms)
    tensors = {k: out.tensors[k].detach() for k in ('position', 'log_scaling', 'rotation')}
    z = 0.5 * torch.randn((plan.n_split, 2, 3), device=device)
    _, dev_ms, wall_ms = timed(lambda: split_children3d(tensors, plan.n_kept, 2, z, 2 ** -0.5), device)
    if r >= warmup:
      times['split3d'][0].append(dev_ms); times['split3d'][1].append(wall_ms)
    moved = bytes_moved(params, plan)
    del out, tensors, plan
  labels = dict(torch='torch path          ', fused='fused step          ', plan='  plan + table      ',
                move='  move + rebuild    ', split3d='  3-D child geometry')
  for name, label in labels.items():
    print(f"{label} device {summary(times[name][0])} | wall {summary(times[name][1])}")
  move_ms = statistics.median(times['move'][0])
  print(f"move: {moved / 1e9:.3f} GB read + written in {move_ms:.3f} ms (events around the launch and the output allocation) "
        f"= {moved / move_ms / 1e9:.2f} TB/s")
  ratio_dev = statistics.median(times['torch'][0]) / statistics.median(times['fused'][0])
  ratio_wall = statistics.median(times['torch'][1]) / statistics.median(times['fused'][1])
  print(f"torch / fused: device {ratio_dev:.2f}x, wall {ratio_wall:.2f}x")
  return ratio_dev, ratio_wall


def main():
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--rows', type=int, nargs='+', default=[6_000_000, 100_000])
  p.add_argument('--rounds', type=int, default=7)
  p.add_argument('--warmup', type=int, default=2)
  args = p.parse_args()
  if not torch.cuda.is_available():
    sys.exit("bench_densify: no GPU visible (there is no CPU fallback to time)")
  device = torch.device('cuda:0')
  print(f"{torch.cuda.get_device_name(device)}; torch {torch.__version__}")
  slower = []
  for n in args.rows:
    ratio_dev, ratio_wall = run(n, args.rounds, args.warmup, device)
    if ratio_wall < 1.0 or ratio_dev < 1.0:
      slower.append(n)
  if slower:
    print(f"FUSED PATH SLOWER THAN THE TORCH PATH at {slower} rows")
    sys.exit(1)


if __name__ == '__main__':
  main()
