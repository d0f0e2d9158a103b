#!/usr/bin/env python
"""k-means assignment, update and a whole compress_scene (csrc/kmeans.hip) at the size of a large scene: N = 6 M rows,
K = 4096 codes, D = 45 (SH degree 3), then D = 24 and 9 (degrees 2 and 1).

Per D, events on the stream, warm-up rounds first, the variants alternating inside every round, median / min / max:

  assign                ms_kmeans_assign: codebook image + norms, then the MFMA arg-min kernel (index and dist2)
  cdist + argmin        the torch baseline: torch.cdist + argmin over row chunks of --chunk points (default 65 536:
                        a 65 536 x 4096 float32 distance block is 1 GiB, written and read back once per chunk)
  mm + argmin           a second torch baseline: (||c||^2 - 2 x c^T).argmin over the same chunks, the GEMM left to
                        torch's BLAS
  update                ms_kmeans_update with the assignment above (sort, chunk sums in float64, combine)
  index_add (float64)   the torch baseline of the update: zeros(K, D).index_add_(0, index, x.double()) / counts

The baselines never call the code under test.  Assignment work is 2 N K D floating-point operations (the multiply-adds of
the score GEMM; norms and the arg-min are not counted); the rate is printed beside the 155 TFLOP/s the f32-input MFMA
sustains on this chip.  The agreement of the kernel's assignment with the cdist baseline's is printed (they may differ
where two codes tie to within rounding).  At D = 45 a whole compress_scene (10 Lloyd iterations, host clock around a
synchronise) is timed once after one warm-up call at a small size.

    python tools/bench_kmeans.py [--n 6000000] [--k 4096] [--dims 45 24 9] [--rounds 5] [--warmup 2] [--chunk 65536]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from taichi_splatting_amd import Gaussians3D, compress_scene                                       # noqa: E402
from taichi_splatting_amd.misc import kmeans as km                                                 # noqa: E402

MFMA_F32_TFLOPS = 155.0       # measured f32-input MFMA peak of the chip (microarchitecture notes)


def event_ms(fn):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end)


def summary(xs):
  return f"median {statistics.median(xs):9.3f} ms  min {min(xs):9.3f}  max {max(xs):9.3f}"


def cdist_argmin(x, codebook, out, chunk):
  for i in range(0, x.shape[0], chunk):
    out[i:i + chunk] = torch.cdist(x[i:i + chunk], codebook).argmin(dim=1)


def mm_argmin(x, codebook, out, chunk):
  norms = (codebook * codebook).sum(dim=1)
  ct = codebook.t().contiguous()
  for i in range(0, x.shape[0], chunk):
    out[i:i + chunk] = torch.addmm(norms, x[i:i + chunk], ct, alpha=-2.0).argmin(dim=1)


def index_add_update(x, index, k):
  sums = torch.zeros((k, x.shape[1]), dtype=torch.float64, device=x.device).index_add_(0, index, x.double())
  counts = torch.bincount(index, minlength=k)
  return (sums / counts.clamp(min=1).unsqueeze(1)).float()


def run(n, k, d, rounds, warmup, chunk, gen):
  device = torch.device('cuda:0')
  print(f"== N = {n}, K = {k}, D = {d} (padded to {(d + 7) // 8 * 8}); baseline chunks of {chunk} points")
  centres = torch.randn((k, d), device=device, generator=gen)
  x = (centres[torch.randint(0, k, (n,), device=device, generator=gen)]
       + 0.5 * torch.randn((n, d), device=device, generator=gen)).contiguous()
  codebook = x[torch.randperm(n, device=device, generator=gen)[:k]].contiguous()
  index = torch.empty((n,), dtype=torch.int32, device=device)
  dist2 = torch.empty((n,), dtype=torch.float32, device=device)
  counts = torch.empty((k,), dtype=torch.int32, device=device)
  base_index, mm_index = (torch.empty((n,), dtype=torch.int64, device=device) for _ in range(2))
  sa = torch.empty((km.assign_scratch_bytes(n, d, k),), dtype=torch.uint8, device=device)
  su = torch.empty((km.update_scratch_bytes(n, d, k),), dtype=torch.uint8, device=device)
  moved = codebook.clone()

  km.kmeans_assign_into(x, codebook, index, dist2, sa)
  index64 = index.long()

  def update():
    moved.copy_(codebook)
    km.kmeans_update_into(x, index, moved, counts, su)

  variants = {
    'assign': lambda: km.kmeans_assign_into(x, codebook, index, dist2, sa),
    'cdist + argmin': lambda: cdist_argmin(x, codebook, base_index, chunk),
    'mm + argmin': lambda: mm_argmin(x, codebook, mm_index, chunk),
    'update': update,
    'index_add (float64)': lambda: index_add_update(x, index64, k),
  }
  times = {key: [] for key in variants}
  for r in range(warmup + rounds):
    for key, fn in variants.items():
      ms = event_ms(fn)
      if r >= warmup:
        times[key].append(ms)
  for key, xs in times.items():
    print(f"{key:20s} {summary(xs)}")
  med = {key: statistics.median(xs) for key, xs in times.items()}
  flop = 2.0 * n * k * d
  for key in ('assign', 'cdist + argmin', 'mm + argmin'):
    tf = flop / med[key] / 1e9
    print(f"{key:20s} {tf:7.1f} TFLOP/s of 2 N K D = {flop / 1e12:.2f} TFLOP: {100 * tf / MFMA_F32_TFLOPS:5.1f} % of the "
          f"{MFMA_F32_TFLOPS:.0f} TFLOP/s f32 MFMA peak (a whole-call rate)")
  print(f"assign vs cdist + argmin: {med['cdist + argmin'] / med['assign']:.2f} x; vs mm + argmin: "
        f"{med['mm + argmin'] / med['assign']:.2f} x; update vs index_add: {med['index_add (float64)'] / med['update']:.2f} x")
  same = float((index64 == base_index).double().mean())
  reference = index_add_update(x, index64, k)
  print(f"agreement with the cdist baseline's assignment: {100 * same:.4f} % of the points; update vs the float64 "
        f"index_add mean: max |difference| {float((moved - reference).abs().max()):.3e}")
  return x


def scene_run(x, k):
  """One compress_scene at the rows of ``x`` (N, 45): host clock around a synchronise, after a warm-up at 100 000 rows"""
  n, device = x.shape[0], x.device

  def scene(rows):
    m = rows.shape[0]
    feature = torch.cat([torch.zeros((m, 3, 1), device=device), rows.reshape(m, 3, 15)], dim=2)
    rotation = torch.zeros((m, 4), device=device)
    rotation[:, 3] = 1.0
    return Gaussians3D(position=torch.zeros((m, 3), device=device), log_scaling=torch.zeros((m, 3), device=device),
                       rotation=rotation, alpha_logit=torch.zeros((m, 1), device=device), feature=feature, batch_size=(m,))

  compress_scene(scene(x[:100_000]), sh_codes=min(k, 100_000), iterations=2, seed=0)
  g = scene(x)
  torch.cuda.synchronize()
  start = time.perf_counter()
  c = compress_scene(g, sh_codes=k, iterations=10, seed=0)
  torch.cuda.synchronize()
  seconds = time.perf_counter() - start
  original = sum(t.numel() * 4 for t in g.shape_tensors() + (g.feature,))
  rows = g.feature[:, :, 1:].reshape(n, 45)
  err = ((rows - c.sh_codebook.reshape(k, 45)[c.sh_index.long()]) ** 2).sum(dim=1).double().mean()
  print(f"== compress_scene: N = {n} degree 3, {k} codes, 10 Lloyd iterations (11 assigns, 10 updates, one host read): "
        f"{seconds:.3f} s; {original / 1e6:.1f} MB -> {c.nbytes / 1e6:.1f} MB ({original / c.nbytes:.2f} x); "
        f"mean squared quantisation error per row {float(err):.4f} (mean squared row norm {float((rows ** 2).sum(dim=1).double().mean()):.4f})")


def main():
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--n', type=int, default=6_000_000)
  p.add_argument('--k', type=int, default=4096)
  p.add_argument('--dims', type=int, nargs='+', default=[45, 24, 9])
  p.add_argument('--rounds', type=int, default=5)
  p.add_argument('--warmup', type=int, default=2)
  p.add_argument('--chunk', type=int, default=65536)
  p.add_argument('--no-scene', action='store_true', help="skip the whole compress_scene")
  args = p.parse_args()
  if not torch.cuda.is_available():
    sys.exit("bench_kmeans: no GPU visible (there is no CPU fallback to time)")
  device = torch.device('cuda:0')
  print(f"{torch.cuda.get_device_name(device)}; torch {torch.__version__}")
  gen = torch.Generator(device=device).manual_seed(0)
  for d in args.dims:
    x = run(args.n, args.k, d, args.rounds, args.warmup, args.chunk, gen)
    if d == 45 and not args.no_scene:
      scene_run(x, args.k)
    del x
    torch.cuda.empty_cache()


if __name__ == '__main__':
  main()
