#!/usr/bin/env python
"""Colours of a vector-quantised scene from its stored form (evaluate_sh_coded, csrc/sh_coded.hip) beside the decoded
path, at the size of a large scene: N = 6 M gaussians, K = 4096 codes, SH degree 3.

Events on the stream, warm-up rounds first, the variants alternating inside every round, median / min / max.  Before
every timed call a 512 MiB buffer is overwritten, outside the events: the streams of one call (240 MB for a forward) fit
the 256 MiB Infinity Cache, so without that the second of two forwards in a round reads what the first left there and
looks 0.05 ms faster whichever of the two it is.  A frame's SH pass follows other kernels: it starts cold.

  coded forward           ms_sh_coded_fwd, the bare C call (one launch, no Python between the events): position, dc,
                          index streamed, the 180-byte code row gathered as stored
  evaluate_sh_coded       the operator's forward: the same launch behind its argument checks, so the difference is
                          host time that a longer stream of work hides
  coded backward          ms_sh_coded_bwd: g_dc dense and a 24-byte record per gaussian into code order, then g_codebook
                          summed per code in float64 in plan order
  decode                  CompressedScene.decode(): index_select + cat into the (N, 3, 16) feature tensor
  decoded forward         evaluate_sh_at on that tensor (identity indices, as the renderer calls it)
  decoded backward        its backward (unique indexes: the streaming parameter-gradient kernel) into (N, 3, 16)
  index_add (float32)     what differentiating through decode() adds: zeros(K, 45).index_add_(0, index, g[:, :, 1:])
                          with float atomics, and the strided copy of g[:, :, 0] into the dc gradient

Peak memory is torch.cuda.max_memory_allocated over one forward + backward of each path, above what the stored scene
itself occupies.  Algorithmic bytes: the coded forward streams 12 (position) + 12 (dc) + 4 (index) + 12 (out) = 40 B per
gaussian and gathers 180 B of code row (L2-resident: K rows are 737 KB); the decoded forward streams 192 + 12 + 12 B.

    python tools/bench_sh_coded.py [--n 6000000] [--k 4096] [--rounds 7] [--warmup 2]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from taichi_splatting_amd import CompressedScene, evaluate_sh_at                                   # noqa: E402
from taichi_splatting_amd import spherical_harmonics as shm                                        # noqa: E402


def event_ms(fn):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end)


def summary(xs):
  return f"median {statistics.median(xs):9.3f} ms  min {min(xs):9.3f}  max {max(xs):9.3f}"


def peak_above(fn, device):
  torch.cuda.synchronize()
  torch.cuda.empty_cache()
  torch.cuda.reset_peak_memory_stats(device)
  before = torch.cuda.memory_allocated(device)
  fn()
  torch.cuda.synchronize()
  return torch.cuda.max_memory_allocated(device) - before


def main():
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--n', type=int, default=6_000_000)
  p.add_argument('--k', type=int, default=4096)
  p.add_argument('--rounds', type=int, default=7)
  p.add_argument('--warmup', type=int, default=2)
  args = p.parse_args()
  if not torch.cuda.is_available():
    sys.exit("bench_sh_coded: no GPU visible (there is no CPU fallback to time)")
  device = torch.device('cuda:0')
  n, k = args.n, args.k
  print(f"{torch.cuda.get_device_name(device)}; torch {torch.__version__}; N = {n}, K = {k}, SH degree 3, "
        f"chunks of {shm._lib.SH_CODED_CHUNK} entries")
  gen = torch.Generator(device=device).manual_seed(0)
  rnd = lambda *shape: torch.randn(shape, device=device, generator=gen)
  zeros = lambda *shape: torch.zeros(shape, device=device)
  scene = CompressedScene(position=rnd(n, 3) * 3.0, log_scaling=zeros(n, 3), rotation=zeros(n, 4), alpha_logit=zeros(n, 1),
                          dc=rnd(n, 3) * 0.5, sh_codebook=rnd(k, 3, 15) * 0.3,
                          sh_index=torch.randint(0, k, (n,), device=device, generator=gen, dtype=torch.int32), sh_degree=3)
  cam = torch.tensor([0.5, -9.0, 1.0], device=device)
  g_out = rnd(n, 3)
  plan = shm.make_coded_sh_plan(scene.sh_index, k)
  print(f"plan: {plan.num_chunks} chunks; order, rank and the chunk tables {4 * (2 * n + 2 * plan.num_chunks + k + 1) / 1e6:.1f} MB")
  identity = torch.arange(n, device=device)
  index64 = scene.sh_index.long()

  dc, codebook = scene.dc.detach().requires_grad_(True), scene.sh_codebook.detach().requires_grad_(True)
  state = {'bare': torch.empty((n, 3), device=device)}

  lib, stream = shm._lib.load(), shm._lib.current_stream(device)

  def bare_forward():
    shm._lib.check(lib.ms_sh_coded_fwd(scene.dc.data_ptr(), scene.sh_index.data_ptr(), scene.sh_codebook.data_ptr(),
                                       scene.position.data_ptr(), cam.data_ptr(), n, k, 3, state['bare'].data_ptr(), stream),
                   "ms_sh_coded_fwd")

  def operator_forward():
    state['out'] = shm.evaluate_sh_coded(dc, scene.sh_index, codebook, scene.position, cam, plan=plan)

  def coded_backward():
    dc.grad = codebook.grad = None
    state['out'].backward(g_out, retain_graph=True)

  dec = {}

  def decode():
    dec['feature'] = scene.decode().feature.requires_grad_(True)

  def decoded_forward():
    dec['out'] = evaluate_sh_at(dec['feature'], scene.position, identity, cam, unique_indexes=True)

  def decoded_backward():
    dec['feature'].grad = None
    dec['out'].backward(g_out, retain_graph=True)

  def index_add():
    g = dec['feature'].grad
    dec['g_codebook'] = torch.zeros((k, 45), device=device).index_add_(0, index64, g[:, :, 1:].reshape(n, 45))
    dec['g_dc'] = g[:, :, 0].contiguous()

  variants = {
    'coded forward': bare_forward,
    'evaluate_sh_coded': operator_forward,
    'coded backward': coded_backward,
    'decode': decode,
    'decoded forward': decoded_forward,
    'decoded backward': decoded_backward,
    'index_add (float32)': index_add,
  }
  times = {key: [] for key in variants}
  flush = torch.empty((512 << 20,), dtype=torch.uint8, device=device)
  for r in range(args.warmup + args.rounds):
    for key, fn in variants.items():
      flush.fill_(r & 1)
      ms = event_ms(fn)
      if r >= args.warmup:
        times[key].append(ms)
  med = {key: statistics.median(xs) for key, xs in times.items()}
  for key, xs in times.items():
    print(f"{key:32s} {summary(xs)}")

  stream_coded, gather = 40.0 * n, 180.0 * n
  stream_decoded = (192.0 + 24.0) * n
  key = 'coded forward'
  print(f"{key:32s} {stream_coded / 1e9:.2f} GB streamed + {gather / 1e9:.2f} GB gathered: "
        f"{stream_coded / med[key] / 1e9:.2f} TB/s of streams, {(stream_coded + gather) / med[key] / 1e9:.2f} TB/s with the gathers")
  print(f"{'decoded forward':32s} {stream_decoded / 1e9:.2f} GB streamed: {stream_decoded / med['decoded forward'] / 1e9:.2f} TB/s")
  bwd_coded = (12.0 + 12.0 + 12.0 + 4.0 + 12.0 + 24.0 + 24.0) * n        # position, out, g_out, rank, g_dc; records out and in
  bwd_decoded = (12.0 + 12.0 + 12.0 + 192.0) * n
  print(f"{'coded backward':32s} {bwd_coded / 1e9:.2f} GB algorithmic: {bwd_coded / med['coded backward'] / 1e9:.2f} TB/s")
  print(f"{'decoded backward':32s} {bwd_decoded / 1e9:.2f} GB algorithmic: {bwd_decoded / med['decoded backward'] / 1e9:.2f} TB/s")
  coded_total = med['coded forward'] + med['coded backward']
  decoded_total = med['decode'] + med['decoded forward'] + med['decoded backward'] + med['index_add (float32)']
  print(f"forward + backward: coded {coded_total:.3f} ms; decoded {decoded_total:.3f} ms "
        f"(decode + forward + backward + index_add): {decoded_total / coded_total:.2f} x")

  # agreement and reproducibility
  out = state['out'].detach()
  assert torch.equal(out, state['bare'])
  print(f"colours against the "
        f"decoded forward {float((out - dec['out'].detach()).abs().max()):.3e}")
  coded_backward()
  first = codebook.grad.clone()
  coded_backward()
  print(f"g_codebook: two runs bitwise equal: {torch.equal(first, codebook.grad)}; against the float32 index_add, max |difference| "
        f"{float((first.reshape(k, 45) - dec['g_codebook']).abs().max()):.3e} (largest entry {float(first.abs().max()):.3e})")
  index_add()
  again = dec['g_codebook'].clone()
  index_add()
  print(f"index_add (float32): two runs bitwise equal: {torch.equal(again, dec['g_codebook'])}")

  # peak memory of one forward + backward, above the stored scene (and the plan for the coded path)
  del dec['feature'], dec['out'], dec['g_codebook'], dec['g_dc'], out, first, again
  state.clear()
  dc.grad = codebook.grad = None

  def coded_once():
    dc, codebook = scene.dc.detach().requires_grad_(True), scene.sh_codebook.detach().requires_grad_(True)
    shm.evaluate_sh_coded(dc, scene.sh_index, codebook, scene.position, cam, plan=plan).backward(g_out)

  def decoded_once():
    dc, codebook = scene.dc.detach().requires_grad_(True), scene.sh_codebook.detach().requires_grad_(True)
    feature = torch.cat([dc.unsqueeze(2), codebook.index_select(0, index64)], dim=2)       # decode(), differentiable
    evaluate_sh_at(feature, scene.position, identity, cam, unique_indexes=True).backward(g_out)

  print(f"peak memory above the stored scene, one forward + backward: coded {peak_above(coded_once, device) / 1e6:.1f} MB; "
        f"through decode() {peak_above(decoded_once, device) / 1e6:.1f} MB (the decoded feature alone: {n * 192 / 1e6:.1f} MB)")


if __name__ == '__main__':
  main()
