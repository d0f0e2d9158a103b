#!/usr/bin/env python
"""Where the time of save_ply / load_ply goes (taichi_splatting_amd/scene_io.py), and the record behind its having no kernel.

Builds a synthetic degree-3 scene of --n gaussians (default 6 000 000: a 1.49 GB file) on the GPU, saves it into a
temporary directory, loads it back to the GPU, checks that every field came back bit for bit, and deletes the file.

  save    gather + copy   per slab: the (rows, 62) table gathered on the device and copied to the host (host seconds,
                          synchronous)
          write           ndarray.tofile of the slabs
  load    read            memory map -> pinned staging buffer (host seconds).  The file was written a moment ago, so this
                          reads the page cache, not a disk: a LOWER bound on what a user waits for
          upload          pinned buffer -> device, device events summed over the slabs
          unpack          the five index_select per slab, device events summed over the slabs
  yardstick               a device-to-device copy of as many bytes as the file's body

    python tools/bench_scene_io.py [--n 6000000] [--chunk-rows 1048576] [--rounds 3]
"""
import argparse
import os
import sys
import tempfile
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from taichi_splatting_amd import Gaussians3D, scene_io                                  # noqa: E402


def main():
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--n', type=int, default=6_000_000)
  p.add_argument('--chunk-rows', type=int, default=1 << 20)
  p.add_argument('--rounds', type=int, default=3)
  args = p.parse_args()
  if not torch.cuda.is_available():
    sys.exit("bench_scene_io: no GPU visible")
  device = torch.device('cuda:0')
  n = args.n
  gen = torch.Generator(device=device).manual_seed(0)
  rand = lambda *shape: torch.randn(shape, device=device, generator=gen)
  scene = Gaussians3D(position=rand(n, 3), log_scaling=rand(n, 3), rotation=rand(n, 4), alpha_logit=rand(n, 1),
                      feature=rand(n, 3, 16) * 0.25, batch_size=(n,))
  body = n * 62 * 4
  print(f"{torch.cuda.get_device_name(device)}; torch {torch.__version__}; N = {n}, SH degree 3, 62 float32 per row, "
        f"body {body / 1e9:.3f} GB, slabs of {args.chunk_rows} rows")

  with tempfile.TemporaryDirectory() as folder:
    path = os.path.join(folder, 'scene.ply')
    for r in range(args.rounds):
      t = {}
      torch.cuda.synchronize()
      start = time.perf_counter()
      scene_io._save(scene, path, args.chunk_rows, t)
      save_s = time.perf_counter() - start
      size = os.path.getsize(path)
      print(f"round {r}  save {save_s:7.3f} s = gather + copy {t['gather_copy_s']:7.3f} + write {t['write_s']:7.3f} "
            f"({size / save_s / 1e9:.2f} GB/s; file {size} bytes)")

      t = {}
      start = time.perf_counter()
      loaded = scene_io._load(path, device, 'file', args.chunk_rows, t)
      torch.cuda.synchronize()
      load_s = time.perf_counter() - start
      device_ms = t['upload_ms'] + t['unpack_ms']
      print(f"round {r}  load {load_s:7.3f} s: read {t['read_s']:7.3f} s ({body / t['read_s'] / 1e9:.2f} GB/s, page cache), "
            f"upload {t['upload_ms']:8.2f} ms ({body / t['upload_ms'] / 1e6:.1f} GB/s), "
            f"unpack {t['unpack_ms']:7.2f} ms ({2 * body / t['unpack_ms'] / 1e6:.0f} GB/s read + written); "
            f"unpack = {100 * t['unpack_ms'] / (load_s * 1e3):.2f} % of the load, upload + unpack = {100 * device_ms / (load_s * 1e3):.1f} %")
      equal = all(torch.equal(getattr(loaded, key).view(torch.int32), getattr(scene, key).view(torch.int32))
                  for key in ('position', 'log_scaling', 'rotation', 'alpha_logit', 'feature'))
      print(f"round {r}  every field bit for bit: {equal}")
      if not equal:
        sys.exit("bench_scene_io: the loaded scene differs from the saved one")
      del loaded
    os.remove(path)

  src = torch.empty((body // 4,), dtype=torch.float32, device=device)
  dst = torch.empty_like(src)
  times = []
  for _ in range(5):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    dst.copy_(src)
    b.record()
    b.synchronize()
    times.append(a.elapsed_time(b))
  print(f"yardstick: device copy of the body's {body / 1e9:.3f} GB: {min(times):.2f} ms ({2 * body / min(times) / 1e6:.0f} GB/s read + written)")


if __name__ == '__main__':
  main()
