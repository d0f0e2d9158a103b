#!/usr/bin/env python
"""Mesh clean-up (csrc/mesh.hip) against its yardsticks — same process, same box, same data.

Workload: the analytic N^3 sphere of tools/bench_tsdf.py (default 512^3) plus a few thousand one-cell shells (single
inside samples on a lattice in the volume's free space), extracted on the device, so that both removal paths do work.

  mesh_components, remove_small_components (min_faces and keep_largest), vertex_normals, each against
    (a) one streaming read of vertices and faces (12 V + 12 T bytes) at the copy rate README.md gives for the box
        (5.0 TB/s), next to a device copy of the same bytes timed here, and
    (b) the most direct torch composition on the GPU: for the labels min-label propagation with scatter_reduce('amin')
        plus pointer jumping until nothing changes (one host read per sweep), for the normals index_add_ of the face
        normals (float32 atomics: not reproducible); results compared first.
  extract_mesh's own time is measured in the same session.

Events on the stream, warm-up, the variants alternating inside every round, median / min / max over the rounds.  Nothing
here is asserted as a ratio; what is slower is printed as slower.

    python tools/bench_mesh.py [--volume 512] [--rounds 10] [--warmup 3] [--lattice 30]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from taichi_splatting_amd import TSDFVolume                           # noqa: E402
from taichi_splatting_amd import mesh as tm                            # noqa: E402

COPY_RATE = 5.0e12          # README.md: "the box copies at 4.6 - 5.4" TB/s


def event_ms(fn):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end)


def interleaved(variants, rounds, warmup):
  times = {k: [] for k in variants}
  for r in range(warmup + rounds):
    for name, fn in variants.items():
      ms = event_ms(fn)
      if r >= warmup:
        times[name].append(ms)
  for name, xs in times.items():
    print(f"  {name:44s} median {statistics.median(xs):9.3f} ms  min {min(xs):9.3f}  max {max(xs):9.3f}")
  return {k: statistics.median(v) for k, v in times.items()}, times


def torch_labels(num_vertices, faces):
  """min-label propagation + pointer jumping; returns (root per vertex = the component's smallest index, sweeps)"""
  index = faces.long()
  flat = index.reshape(-1)
  label = torch.arange(num_vertices, device=faces.device)
  sweeps = 0
  while True:
    sweeps += 1
    face_min = label[index].amin(dim=1)
    new = label.scatter_reduce(0, flat, face_min.repeat_interleave(3), 'amin', include_self=True)
    new = new[new]                                                    # pointer jumping (labels are vertex indices)
    new = new[new]
    if torch.equal(new, label):                                       # the host read of the sweep
      return label, sweeps
    label = new


def torch_normals(vertices, faces):
  index = faces.long()
  a, b, c = vertices[index[:, 0]], vertices[index[:, 1]], vertices[index[:, 2]]
  cross = torch.linalg.cross(b - a, c - a)
  sums = torch.zeros_like(vertices)
  for k in range(3):
    sums.index_add_(0, index[:, k], cross)
  return torch.nn.functional.normalize(sums, dim=1)


def main():
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--volume', type=int, default=512)
  p.add_argument('--rounds', type=int, default=10)
  p.add_argument('--warmup', type=int, default=3)
  p.add_argument('--lattice', type=int, default=30, help="spacing, in samples, of the lattice of one-cell shells")
  args = p.parse_args()
  if not torch.cuda.is_available():
    sys.exit("bench_mesh: no GPU visible (there is no CPU fallback to time)")
  device = torch.device('cuda:0')
  print(f"{torch.cuda.get_device_name(device)}; torch {torch.__version__}")
  n = args.volume
  voxel = 2.0 / (n - 1)
  volume = TSDFVolume((-1.0, -1.0, -1.0), voxel, (n, n, n), colour=False, device=device)
  volume.tsdf.copy_(((volume.positions().norm(dim=-1) - 0.8) / volume.truncation).clamp(-1, 1))
  volume.weight.fill_(1.0)
  sites = torch.arange(args.lattice // 2, n - 1, args.lattice, device=device)
  k, j, i = torch.meshgrid(sites, sites, sites, indexing='ij')
  free = volume.tsdf[k, j, i] >= 1.0                                   # outside the sphere and away from its surface
  volume.tsdf[k[free], j[free], i[free]] = -0.5
  shells = int(free.sum())
  mesh = volume.extract_mesh()
  torch.cuda.synchronize()
  num_vertices, num_faces = mesh.vertices.shape[0], mesh.faces.shape[0]
  stream_bytes = 12 * num_vertices + 12 * num_faces
  read_ms = stream_bytes / COPY_RATE * 1e3
  print(f"== {n}^3 sphere + {shells} one-cell shells: {num_vertices} vertices, {num_faces} triangles; one streaming read of "
        f"vertices and faces ({stream_bytes / 1e6:.1f} MB): {read_ms:.4f} ms at {COPY_RATE / 1e12:.1f} TB/s")

  components = tm.mesh_components(mesh)
  counts = components.face_count.sort(descending=True).values
  shell_faces = int(counts[-1])
  print(f"   {components.num_components} components; the largest {int(counts[0])} faces, the smallest {shell_faces}")
  assert components.num_components == shells + 1
  roots, sweeps = torch_labels(num_vertices, mesh.faces)
  rank = torch.unique(roots, return_inverse=True)[1].to(torch.int32)
  assert torch.equal(rank, components.vertex_label), "the torch composition and the kernel disagree"
  print(f"   torch composition of the labels: {sweeps} sweeps; labels equal the kernel's")
  kernel_normals = tm.vertex_normals(mesh)
  composed_normals = torch_normals(mesh.vertices, mesh.faces)
  print(f"   normals: largest difference between the kernel and the index_add_ composition "
        f"{float((kernel_normals - composed_normals).abs().max()):.3e}")
  cleaned = tm.remove_small_components(mesh, min_faces=shell_faces + 1)
  assert cleaned.faces.shape[0] == int(counts[0])
  largest = tm.remove_small_components(mesh, keep_largest=1)
  assert torch.equal(largest.faces, cleaned.faces)

  src = torch.empty((stream_bytes // 4,), dtype=torch.float32, device=device)
  dst = torch.empty_like(src)
  variants = {
    'extract_mesh (public call)': volume.extract_mesh,
    'mesh_components': lambda: tm.mesh_components(mesh),
    f'remove_small_components(min_faces={shell_faces + 1})': lambda: tm.remove_small_components(mesh, min_faces=shell_faces + 1),
    'remove_small_components(keep_largest=1)': lambda: tm.remove_small_components(mesh, keep_largest=1),
    'vertex_normals': lambda: tm.vertex_normals(mesh),
    'torch: index_add_ normals': lambda: torch_normals(mesh.vertices, mesh.faces),
    'device copy of vertices + faces bytes': lambda: dst.copy_(src),
  }
  median, _ = interleaved(variants, args.rounds, args.warmup)
  print("-- the label composition (fewer rounds: it is the slow one)")
  label_median, _ = interleaved({'torch: amin propagation + pointer jumping': lambda: torch_labels(num_vertices, mesh.faces),
                                 'mesh_components (again, beside it)': lambda: tm.mesh_components(mesh)},
                                max(args.rounds // 3, 3), 1)
  print("-- against the yardsticks (medians)")
  for name, other in (('mesh_components', label_median['torch: amin propagation + pointer jumping']),
                      (f'remove_small_components(min_faces={shell_faces + 1})', None),
                      ('remove_small_components(keep_largest=1)', None),
                      ('vertex_normals', median['torch: index_add_ normals'])):
    line = f"  {name:44s} {median[name]:9.3f} ms = {median[name] / read_ms:7.1f} x one streaming read"
    if other is not None:
      ratio = other / median[name]
      line += f"; torch composition {other:9.3f} ms = {ratio:.2f} x the kernel ({'kernel faster' if ratio > 1 else 'KERNEL SLOWER'})"
    print(line + f"; {median[name] / median['extract_mesh (public call)']:.2f} x extract_mesh")


if __name__ == '__main__':
  main()
