#!/usr/bin/env python
"""Fixed-budget densification (csrc/relocate.hip) against its torch composition, same process, same box.

Scene: the benchmark's shape — N rows x 59 floats in the five Gaussians3D tensors (SH degree 3) with VisibilityAwareAdam
state (two moments per parameter, running visibility, total weight) — with 1 %, 10 % and 50 % of the rows dead.

  relocate   ParameterClass.relocate: weights, torch.cumsum, draw, fresh opacity / scale, one move launch; in place, no
             host read.  The move launch is also timed alone and its bytes counted, to set beside ms_densify_move.
  torch      multinomial (its sample count is a host read) + bincount + the opacity / scale correction on the drawn rows
             + one indexed copy per tensor and one indexed fill per state tensor.
  perturb    ms_perturb_positions against the torch chain (normalise, rotation matrices, two bmm, sigmoid gate, add_);
             its 68 bytes per row set beside a device copy of the same bytes.

The two relocation paths draw with different samplers, so they are compared by what they must agree on (every dead row
moved onto a live one), not bit for bit.  Per path, after warm-up, alternating: device time (events on the stream) and
wall time (host clock to a device synchronise).

    python tools/bench_relocate.py [--rows 6000000] [--dead 0.01 0.1 0.5] [--rounds 7] [--warmup 2]
"""
import argparse
import ctypes
import math
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from taichi_splatting_amd import _lib                                                # noqa: E402
from taichi_splatting_amd.misc.relocate import perturb_positions                     # noqa: E402
from taichi_splatting_amd.optim import ParameterClass, VisibilityAwareAdam           # noqa: E402
from taichi_splatting_amd.optim.relocate import binomial_table, logit_threshold      # noqa: E402

SHAPES = dict(position=(3,), log_scaling=(3,), rotation=(4,), alpha_logit=(1,), feature=(3, 16))
MIN_OPACITY = 0.005


def make_params(n, device):
  g = torch.Generator(device=device).manual_seed(n)
  tensors = {k: torch.randn((n, *s), device=device, generator=g) for k, s in SHAPES.items()}
  tensors['log_scaling'] = tensors['log_scaling'] * 0.5 - 3.0
  params = ParameterClass(tensors, {k: dict(lr=1e-3) for k in SHAPES}, optimizer=VisibilityAwareAdam)
  for k in SHAPES:
    params.tensors[k].grad = torch.randn((n, *SHAPES[k]), device=device, generator=g)
  params.step(indexes=None, visibility=torch.rand(n, device=device, generator=g) + 0.1)     # creates every state tensor
  params.zero_grad()
  return params


def torch_relocate(params, binomials):
  """3DGS-MCMC relocation as torch ops on the same ParameterClass, in place."""
  threshold = logit_threshold(MIN_OPACITY)
  with torch.no_grad():
    alpha, log_scaling = params.tensors['alpha_logit'].detach(), params.tensors['log_scaling'].detach()
    a = alpha.squeeze(1)
    dead = ~(a > threshold)
    dead_idx = dead.nonzero().squeeze(1)                   # host read: the number of dead rows
    if dead_idx.numel() == 0:
      return 0
    probs = torch.sigmoid(a).masked_fill(dead, 0.0)
    picked = torch.multinomial(probs, dead_idx.numel(), replacement=True)
    count = torch.bincount(picked, minlength=a.shape[0])
    drawn_idx = (count > 0).nonzero().squeeze(1)           # host read
    ratio = (count[drawn_idx] + 1).clamp(max=_lib.RELOCATE_MAX_RATIO)
    o = torch.sigmoid(a[drawn_idx].double())
    new = 1.0 - (1.0 - o) ** (1.0 / ratio.double())
    denom, p = torch.zeros_like(o), torch.ones_like(o)
    columns = binomials.cumsum(0)                          # columns[m, k] = sum_{i <= m} C(i, k)
    for k in range(int(ratio.max())):
      p = p * new
      term = p / math.sqrt(k + 1) * columns[ratio - 1, k]
      denom = denom + (term if k % 2 == 0 else -term)
    clamped = new.clamp(MIN_OPACITY, 1.0 - 1e-7)
    alpha[drawn_idx] = torch.log(clamped / (1.0 - clamped)).float().unsqueeze(1)
    log_scaling[drawn_idx] = (log_scaling[drawn_idx].double() + torch.log(o / denom).unsqueeze(1)).float()
    for t in params.tensors.values():
      t.detach()[dead_idx] = t.detach()[picked]
    for st in params.tensor_state.values():
      for key, t in st.items():
        if key == 'running_vis':
          t[dead_idx] = t[picked]
        else:
          t[dead_idx] = 0
          t[drawn_idx] = 0
    return dead_idx.numel()


def torch_perturb(params, step, z, k=100.0, x0=0.995):
  with torch.no_grad():
    t = {name: params.tensors[name].detach() for name in ('position', 'log_scaling', 'rotation', 'alpha_logit')}
    q = t['rotation'] / t['rotation'].norm(dim=1, keepdim=True)
    x, y, zz, w = q.unbind(1)
    R = torch.stack([1 - 2 * y * y - 2 * zz * zz, 2 * x * y - 2 * w * zz, 2 * x * zz + 2 * w * y,
                     2 * x * y + 2 * w * zz, 1 - 2 * x * x - 2 * zz * zz, 2 * y * zz - 2 * w * x,
                     2 * x * zz - 2 * w * y, 2 * y * zz + 2 * w * x, 1 - 2 * x * x - 2 * y * y], 1).view(-1, 3, 3)
    sigma = torch.bmm(R * torch.exp(2.0 * t['log_scaling']).unsqueeze(1), R.transpose(1, 2))
    gate = torch.sigmoid(k * ((1.0 - torch.sigmoid(t['alpha_logit'])) - x0))
    t['position'].add_(torch.bmm(sigma, z.unsqueeze(2)).squeeze(2) * gate * step)


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


def move_descriptors(params, fresh_opacity, fresh_scale):
  arrays = []
  for name, t in params.tensors.items():
    role = _lib.RELOCATE_OPACITY if name == 'alpha_logit' else _lib.RELOCATE_SCALE if name == 'log_scaling' else _lib.RELOCATE_COPY
    arrays.append((t.detach(), role))
  for st in params.tensor_state.values():
    for key, t in st.items():
      arrays.append((t, _lib.RELOCATE_INHERIT if key == 'running_vis' else _lib.RELOCATE_ZERO_TOUCHED))
  n = arrays[0][0].shape[0]
  descriptors = (_lib.RelocateArrayC * len(arrays))()
  for d, (t, role) in zip(descriptors, arrays):
    d.struct_size, d.role, d.data = ctypes.sizeof(_lib.RelocateArrayC), role, t.data_ptr()
    d.row_bytes = (t.numel() // n) * t.element_size()
    if role == _lib.RELOCATE_OPACITY:
      d.fresh = fresh_opacity.data_ptr()
    elif role == _lib.RELOCATE_SCALE:
      d.fresh = fresh_scale.data_ptr()
  return descriptors, arrays


def bytes_moved(arrays, n, moved, drawn):
  """Bytes the move launch has to read and write: 8 bytes of table per row of the scene; per moved row a row read and a
  row written (moments: written only); per drawn row its moments, opacity and scale written and the latter two read."""
  total = 8 * n
  for t, role in arrays:
    row = (t.numel() // n) * t.element_size()
    if role == _lib.RELOCATE_ZERO_TOUCHED:
      total += row * (moved + drawn)
    elif role in (_lib.RELOCATE_OPACITY, _lib.RELOCATE_SCALE):
      total += 2 * row * (moved + drawn)
    else:
      total += 2 * row * moved
  return total


def run(n, fraction, rounds, warmup, device, params):
  g = torch.Generator(device=device).manual_seed(int(fraction * 1000) + 1)
  alive = params.tensors['alpha_logit'].detach().clone().clamp_(min=-4.0)
  dead = torch.rand(n, device=device, generator=g) < fraction
  start_alpha = torch.where(dead.unsqueeze(1), torch.full_like(alive, -10.0), alive)
  words = torch.randint(torch.iinfo(torch.int64).min, torch.iinfo(torch.int64).max, (n,), device=device, generator=g)
  binomials = torch.tensor(binomial_table(), dtype=torch.float64).to(device)
  state_floats = sum(t.numel() // n for st in params.tensor_state.values() for t in st.values())
  print(f"== {n} rows x {sum(t.numel() // n for t in params.tensors.values())} parameter floats + {state_floats} state floats; "
        f"{int(dead.sum())} dead ({100 * fraction:g} %)")

  def reset():
    params.tensors['alpha_logit'].detach().copy_(start_alpha)

  lib, stream = _lib.load(), _lib.current_stream(device)
  fresh_opacity, fresh_scale = torch.zeros(n, device=device), torch.zeros(n, 3, device=device)
  times = dict(relocate=([], []), torch=([], []), move=([], []))
  for r in range(warmup + rounds):
    reset()
    result, dev_ms, wall_ms = timed(lambda: params.relocate(min_opacity=MIN_OPACITY, random=words, inherit_state=('running_vis',)), device)
    if r >= warmup:
      times['relocate'][0].append(dev_ms); times['relocate'][1].append(wall_ms)
    n_dead, n_drawn, _ = result.counts.tolist()
    assert n_dead == int(dead.sum()) and int((result.src != torch.arange(n, device=device)).sum()) == n_dead
    # the move launch alone, on the tables of that call (it moves the same rows again: the same bytes)
    descriptors, arrays = move_descriptors(params, fresh_opacity, fresh_scale)
    _, dev_ms, wall_ms = timed(lambda: _lib.check(lib.ms_relocate_move(descriptors, len(arrays), result.src.data_ptr(),
                                                                     result.count.data_ptr(), n, stream), "move"), device)
    if r >= warmup:
      times['move'][0].append(dev_ms); times['move'][1].append(wall_ms)
    moved_bytes = bytes_moved(arrays, n, n_dead, n_drawn)
    reset()
    torch_dead, dev_ms, wall_ms = timed(lambda: torch_relocate(params, binomials), device)
    assert torch_dead == n_dead
    if r >= warmup:
      times['torch'][0].append(dev_ms); times['torch'][1].append(wall_ms)
  labels = dict(torch='torch composition   ', relocate='relocate            ', move='  move launch alone ')
  for name, label in labels.items():
    print(f"{label} device {summary(times[name][0])} | wall {summary(times[name][1])}")
  move_ms = statistics.median(times['move'][0])
  print(f"move: {n_dead} rows moved, {n_drawn} drawn; {moved_bytes / 1e9:.3f} GB read + written in {move_ms:.3f} ms "
        f"= {moved_bytes / move_ms / 1e9:.2f} TB/s")
  ratio_dev = statistics.median(times['torch'][0]) / statistics.median(times['relocate'][0])
  ratio_wall = statistics.median(times['torch'][1]) / statistics.median(times['relocate'][1])
  print(f"torch / relocate: device {ratio_dev:.2f}x, wall {ratio_wall:.2f}x")
  return ratio_dev, ratio_wall


def run_perturb(n, rounds, warmup, device, params):
  g = torch.Generator(device=device).manual_seed(5)
  z = torch.randn(n, 3, device=device, generator=g)
  params.tensors['alpha_logit'].detach().copy_(4.0 * torch.randn(n, 1, device=device, generator=g) - 2.0)
  src, dst = torch.empty(n * 14, device=device), torch.empty(n * 14, device=device)      # 56 bytes per row
  times = dict(perturb=([], []), torch=([], []), copy=([], []))
  for r in range(warmup + rounds):
    for name, fn in (('perturb', lambda: perturb_positions(params, 1e-3, z=z)), ('torch', lambda: torch_perturb(params, 1e-3, z)),
                     ('copy', lambda: dst.copy_(src))):
      _, dev_ms, wall_ms = timed(fn, device)
      if r >= warmup:
        times[name][0].append(dev_ms); times[name][1].append(wall_ms)
  print(f"== position noise, {n} rows")
  labels = dict(torch='torch composition   ', perturb='ms_perturb_positions', copy='copy of 56 B per row')
  for name, label in labels.items():
    print(f"{label} device {summary(times[name][0])} | wall {summary(times[name][1])}")
  ms = statistics.median(times['perturb'][0])
  moved = 68 * n                                           # 56 bytes read, 12 written
  copy_ms = statistics.median(times['copy'][0])
  print(f"perturb: {moved / 1e9:.3f} GB read + written in {ms:.3f} ms = {moved / ms / 1e9:.2f} TB/s; "
        f"the copy: {112 * n / 1e9:.3f} GB in {copy_ms:.3f} ms = {112 * n / copy_ms / 1e9:.2f} TB/s")
  ratio = statistics.median(times['torch'][0]) / ms
  print(f"torch / perturb: device {ratio:.2f}x")
  return ratio


def main():
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--rows', type=int, default=6_000_000)
  p.add_argument('--dead', type=float, nargs='+', default=[0.01, 0.1, 0.5])
  p.add_argument('--rounds', type=int, default=7)
  p.add_argument('--warmup', type=int, default=2)
  args = p.parse_args()
  if not torch.cuda.is_available():
    sys.exit("bench_relocate: no GPU visible (there is no CPU fallback to time)")
  device = torch.device('cuda:0')
  print(f"{torch.cuda.get_device_name(device)}; torch {torch.__version__}")
  params = make_params(args.rows, device)
  slower = []
  for fraction in args.dead:
    ratio_dev, ratio_wall = run(args.rows, fraction, args.rounds, args.warmup, device, params)
    if ratio_dev < 1.0 or ratio_wall < 1.0:
      slower.append(f"{100 * fraction:g} % dead")
  if run_perturb(args.rows, args.rounds, args.warmup, device, params) < 1.0:
    slower.append("perturb")
  if slower:
    print(f"KERNELS SLOWER THAN THE TORCH COMPOSITION at {slower}")
    sys.exit(1)


if __name__ == '__main__':
  main()
