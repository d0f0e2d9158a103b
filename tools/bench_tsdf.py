#!/usr/bin/env python
"""TSDF fusion and mesh extraction (csrc/tsdf.hip) against their yardsticks — same process, same box, same data.

  integrate   a coloured N^3 volume (default 512^3, 2.7 GB) and S^2 frames (default 2048^2), C = 1 and C = 8 frames per
              call, with frusta that cover the whole volume and about a tenth of it, against
                - the float32 torch composition of the same rule on the GPU (tests/tsdf_oracle.integrate; results compared
                  first), one pass over the volume per frame with its temporaries, and
                - the byte floor: 40 B per touched sample and call (tsdf, weight and colour read and written once) at the
                  copy rate README.md gives for the box (5.0 TB/s, the middle of its 4.6 - 5.4), next to a device copy of
                  the same bytes timed here.
  extract     classify, the two scans and emit of extract_mesh timed apart (the C entry points, events) on an analytic
              sphere and on a volume fused from eight rendered sphere depth frames, against one streaming read of tsdf and
              weight (8 B per sample at the same rate), and the whole public call with its host read.

Events on the stream, warm-up, the variants alternating inside every round, median / min / max over the rounds; "faster"
holds only when the kernel's slowest round beats the composition's fastest.  Nothing here is asserted as a ratio.

    python tools/bench_tsdf.py [--volume 512] [--image 2048] [--rounds 10] [--warmup 3]
"""
import argparse
import ctypes
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from taichi_splatting_amd import TSDFVolume, _lib                    # noqa: E402
from tests import tsdf_oracle as to                                   # noqa: E402

COPY_RATE = 5.0e12          # README.md: "the box copies at 4.6 - 5.4" TB/s
SAMPLE_BYTES = 40


def event_ms(fn):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end)


def summary(xs):
  return f"median {statistics.median(xs):9.3f} ms  min {min(xs):9.3f}  max {max(xs):9.3f}"


def interleaved(variants, rounds, warmup):
  times = {k: [] for k in variants}
  for r in range(warmup + rounds):
    for name, fn in variants.items():
      ms = event_ms(fn)
      if r >= warmup:
        times[name].append(ms)
  for name, xs in times.items():
    print(f"  {name:34s} {summary(xs)}")
  return times


def cameras_around(count, size, zoom, device):
  """``count`` cameras on a circle of radius 4 around the unit-cube-sized volume at the origin; zoom 1 sees all of it"""
  rows = []
  for c in range(count):
    angle = 0.3 + 2.0 * math.pi * c / max(count, 1)
    eye = 4.0 * torch.tensor([math.cos(angle), 0.17, math.sin(angle)]).numpy()
    focal = zoom * size / (2.0 * math.tan(math.radians(20.0)))
    rows.append(to.pack_camera(to.look_at(eye, (0.01, -0.02, 0.03), roll=0.1 * c), focal, focal, 0.5 * size + 0.3,
                               0.5 * size - 0.2, 0.5, 20.0, size, size))
  return torch.stack(rows).to(device)


def sphere_depth(cameras, size, radius, device):
  """(C, S, S) camera-z depth of the sphere of ``radius`` at the origin, 0 where the ray misses it"""
  out = []
  ys, xs = torch.meshgrid(torch.arange(size, device=device, dtype=torch.float32) + 0.5,
                          torch.arange(size, device=device, dtype=torch.float32) + 0.5, indexing='ij')
  for row in cameras:
    T = row[:12].reshape(3, 4)
    rotation, translation = T[:, :3], T[:, 3]
    eye = -rotation.T @ translation
    ray_cam = torch.stack([(xs - row[14]) / row[12], (ys - row[15]) / row[13], torch.ones_like(xs)], dim=-1)      # z = 1
    ray = ray_cam @ rotation                                              # world direction per unit camera z
    a = (ray * ray).sum(-1)
    b = 2.0 * (ray @ eye)
    c = float(eye @ eye) - radius * radius
    disc = b * b - 4.0 * a * c
    hit = disc > 0
    out.append(torch.where(hit, (-b - disc.clamp(min=0).sqrt()) / (2.0 * a), torch.zeros_like(a)))
  return torch.stack(out)


def bench_integrate(n, size, rounds, warmup, device):
  voxel = 2.0 / (n - 1)
  origin = (-1.0, -1.0, -1.0)
  volume = TSDFVolume(origin, voxel, (n, n, n), device=device)
  samples = volume.num_samples
  generator = torch.Generator(device=device).manual_seed(0)
  src = torch.empty((samples * SAMPLE_BYTES // 8,), dtype=torch.float32, device=device)
  dst = torch.empty_like(src)
  slower = []
  for label, zoom in (('whole volume in view', 0.45), ('about a tenth in view', 4.5)):
    cameras = cameras_around(8, size, zoom, device)
    depth = sphere_depth(cameras, size, 0.8, device)
    depth = torch.where(depth > 0, depth, torch.full_like(depth, 4.0))         # every pixel fuses: the whole frustum is touched
    image = torch.rand((8, size, size, 3), device=device, generator=generator)
    # how much of the volume the frusta touch, and the comparison of the results (one frame, fresh volumes)
    volume.reset()
    volume.integrate(depth[:1], cameras[:1], colour=image[:1])
    fresh = (torch.ones_like(volume.tsdf), torch.zeros_like(volume.weight), torch.zeros_like(volume.colour))
    want = to.integrate(*fresh, origin, voxel, volume.truncation, None, depth[:1], cameras[:1], image[:1], dtype=torch.float32)
    del fresh
    same = (volume.tsdf == want[0]) & (volume.weight == want[1]) & (volume.colour == want[2]).all(-1)
    close = ((volume.tsdf - want[0]).abs() <= 1e-5) & (volume.weight == want[1])
    touched_one = float((volume.weight > 0).float().mean())
    print(f"== integrate, {n}^3 coloured volume, {size}^2 frames, {label}: one frame touches {100 * touched_one:.1f} % of the samples; "
          f"kernel against the float32 composition: {100 * float(same.float().mean()):.5f} % of the samples bitwise equal, "
          f"{100 * float(close.float().mean()):.5f} % within 1e-5")
    assert float(close.float().mean()) > 0.9999
    del want, same, close
    volume.reset()
    volume.integrate(depth, cameras, colour=image)
    touched_all = float((volume.weight > 0).float().mean())
    for count in (1, 8):
      touched = touched_one if count == 1 else touched_all
      floor_ms = samples * touched * SAMPLE_BYTES / COPY_RATE * 1e3
      variants = {
        f'fused, C = {count}': lambda: volume.integrate(depth[:count], cameras[:count], colour=image[:count]),
        f'torch composition, C = {count}': lambda: to.integrate(volume.tsdf, volume.weight, volume.colour, origin, voxel,
                                                                 volume.truncation, None, depth[:count], cameras[:count],
                                                                 image[:count], dtype=torch.float32),
        'copy of 40 B per sample (all)': lambda: dst.copy_(src),
      }
      print(f"-- C = {count}: touches {100 * touched:.1f} % of the samples; byte floor {floor_ms:.3f} ms at {COPY_RATE / 1e12:.1f} TB/s")
      times = interleaved(variants, max(rounds // (2 if count == 8 else 1), 3), warmup)
      fused, composed = times[f'fused, C = {count}'], times[f'torch composition, C = {count}']
      med = statistics.median(fused)
      outside = max(fused) < min(composed)
      print(f"  fused: {med / floor_ms:.2f} x the byte floor, {samples * touched * SAMPLE_BYTES / med / 1e9:.2f} TB/s on the touched bytes; "
            f"composition / fused {statistics.median(composed) / med:.1f} x; the fused call's slowest round "
            f"{'beats' if outside else 'DOES NOT beat'} the composition's fastest")
      if not outside:
        slower.append(f'{label}, C = {count}')
      if count == 8:
        print(f"  eight frames in one call cost {med / one_frame:.2f} x one frame ({med:.3f} against {one_frame:.3f} ms)")
      else:
        one_frame = med
  return slower


def bench_extract(n, size, rounds, warmup, device):
  lib = _lib.load()
  voxel = 2.0 / (n - 1)
  origin = (-1.0, -1.0, -1.0)
  volume = TSDFVolume(origin, voxel, (n, n, n), colour=True, device=device)
  samples = volume.num_samples
  read_ms = samples * 8 / COPY_RATE * 1e3
  word = torch.empty((samples,), dtype=torch.int32, device=device)
  vscan = torch.empty((samples + 1,), dtype=torch.int32, device=device)
  tscan = torch.empty((samples + 1,), dtype=torch.int32, device=device)
  stream = _lib.current_stream(volume.device)
  scan_call = lambda scan: lambda tmp, size: lib.ms_exclusive_scan_i32(
    scan.data_ptr(), samples, scan.data_ptr(), None, tmp, size, stream)
  tmp = _lib.scratch_block(_lib.scratch_bytes(scan_call(vscan), "scan"), device)
  origin_c = (ctypes.c_double * 3)(*origin)

  def classify():
    _lib.check(lib.ms_tsdf_classify(volume.tsdf.data_ptr(), volume.weight.data_ptr(), n, n, n, 0.0, word.data_ptr(),
                                    vscan.data_ptr(), tscan.data_ptr(), stream), "classify")

  def scans():
    for scan in (vscan, tscan):
      _lib.run_in_scratch(scan_call(scan), tmp, "scan")

  for label in ('analytic sphere', 'fused sphere frames'):
    volume.reset()
    if label == 'analytic sphere':
      volume.tsdf.copy_(((volume.positions().norm(dim=-1) - 0.8) / volume.truncation).clamp(-1, 1))
      volume.weight.fill_(1.0)
    else:
      cameras = cameras_around(8, size, 0.45, device)
      depth = sphere_depth(cameras, size, 0.8, device)
      volume.integrate(depth, cameras, colour=torch.rand((8, size, size, 3), device=device))
    mesh = volume.extract_mesh()
    v, t = mesh.vertices.shape[0], mesh.faces.shape[0]
    radial = (mesh.vertices.norm(dim=1) - 0.8).abs()
    print(f"== extract_mesh, {n}^3, {label}: {v} vertices, {t} triangles; radial error median {float(radial.median()) / voxel:.4f} h, "
          f"max {float(radial.max()) / voxel:.4f} h; one streaming read of tsdf and weight: {read_ms:.3f} ms at {COPY_RATE / 1e12:.1f} TB/s")
    vertices, faces, colours = torch.empty_like(mesh.vertices), torch.empty_like(mesh.faces), torch.empty_like(mesh.colours)

    def emit():
      _lib.check(lib.ms_tsdf_emit(volume.tsdf.data_ptr(), volume.weight.data_ptr(), volume.colour.data_ptr(), n, n, n, origin_c,
                                  voxel, 0.0, word.data_ptr(), vscan.data_ptr(), tscan.data_ptr(), vertices.data_ptr(),
                                  faces.data_ptr(), colours.data_ptr(), stream), "emit")

    # the stages depend on each other: they run in order inside every round, each under its own pair of events
    times = interleaved({'classify': classify, 'two scans': scans, 'emit': emit, 'extract_mesh (public call)': volume.extract_mesh},
                        rounds, warmup)
    assert torch.equal(vertices, mesh.vertices) and torch.equal(faces, mesh.faces)
    total = sum(statistics.median(times[k]) for k in ('classify', 'two scans', 'emit'))
    print(f"  classify + scans + emit {total:.3f} ms = {total / read_ms:.1f} x one streaming read of the volume")


def main():
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--volume', type=int, default=512)
  p.add_argument('--image', type=int, default=2048)
  p.add_argument('--rounds', type=int, default=10)
  p.add_argument('--warmup', type=int, default=3)
  p.add_argument('--skip-extract', action='store_true')
  args = p.parse_args()
  if not torch.cuda.is_available():
    sys.exit("bench_tsdf: no GPU visible (there is no CPU fallback to time)")
  device = torch.device('cuda:0')
  print(f"{torch.cuda.get_device_name(device)}; torch {torch.__version__}")
  slower = bench_integrate(args.volume, args.image, args.rounds, args.warmup, device)
  if not args.skip_extract:
    bench_extract(args.volume, args.image, args.rounds, args.warmup, device)
  if slower:
    print(f"FUSED CALL NOT FASTER THAN THE TORCH COMPOSITION OUTSIDE THE SPREAD: {slower}")
    sys.exit(1)


if __name__ == '__main__':
  main()
