#!/usr/bin/env python
"""Mesh simplification (csrc/mesh_simplify.hip) against its yardsticks — same process, same box, same data.

Workload: the mesh of tools/bench_mesh.py — the analytic N^3 sphere (default 512^3) plus a few thousand one-cell shells,
extracted on the device — simplified at cells of 2, 4 and 8 voxels.

  simplify_mesh (quadric and mean placement), whole call and stage by stage (an event after every stage of
    mesh._simplify; the stages between the two host reads are sorts, scans and the kernels of mesh_simplify.hip), against
    (a) one streaming read of vertices and faces (12 V + 12 T bytes) at the copy rate README.md gives for the box
        (5.0 TB/s), next to a device copy of the same bytes timed here,
    (b) the most direct torch composition on the GPU: torch.unique of the cell keys, float64 index_add_ of the means and
        the quadrics (float64 atomics: not reproducible), batched torch.linalg.solve, the in-cell test, torch.unique of the
        packed triples; vertex and face counts compared first, positions to the figure printed, and
    (c) for the placement kernel alone, the bytes its gathers name — per corner the corner index, the face row and three
        vertex rows (4 + 12 + 36 bytes), per member the index and the row (4 + 12) — at the same copy rate.

Events on the stream, warm-up, the variants alternating inside every round, median / min / max over the rounds.  Nothing
here is asserted as a ratio; what is slower is printed as slower.

    python tools/bench_mesh_simplify.py [--volume 512] [--rounds 5] [--warmup 2] [--lattice 30] [--cells 2 4 8]
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
  return {k: statistics.median(v) for k, v in times.items()}


def staged(mesh, cell_size, placement, rounds, warmup):
  """median ms of every stage of mesh._simplify (events recorded where it reports a stage)"""
  names, samples = [], {}
  for r in range(warmup + rounds):
    marks = [('start', torch.cuda.Event(enable_timing=True))]
    marks[0][1].record()

    def stage(name):
      event = torch.cuda.Event(enable_timing=True)
      event.record()
      marks.append((name, event))

    tm._simplify(mesh, cell_size, None, placement, 1e-3, stage=stage)
    torch.cuda.synchronize()
    if r >= warmup:
      for (_, before), (name, after) in zip(marks[:-1], marks[1:]):
        if name not in samples:
          names.append(name)
        samples.setdefault(name, []).append(before.elapsed_time(after))
  return [(name, statistics.median(samples[name])) for name in names]


def torch_simplify(vertices, faces, origin, cell_size, regularisation=1e-3):
  """the rules of simplify_mesh by torch calls; returns (vertices, faces)"""
  device = vertices.device
  index = faces.long()
  size = torch.tensor(cell_size, dtype=torch.float32, device=device)
  cell = torch.floor((vertices - origin) / size).long()
  key = (cell[:, 2] << 42) | (cell[:, 1] << 21) | cell[:, 0]
  referenced = torch.zeros((vertices.shape[0],), dtype=torch.bool, device=device)
  referenced[index.reshape(-1)] = True
  key = torch.where(referenced, key, torch.full_like(key, 2 ** 63 - 1))
  unique_keys, cluster = torch.unique(key, return_inverse=True)        # sorted: ascending keys; the sentinel, if any, last
  count = unique_keys.shape[0]
  p64 = vertices.double()
  members = torch.zeros((count,), dtype=torch.float64, device=device).index_add_(0, cluster, torch.ones_like(p64[:, 0]))
  mean = torch.zeros((count, 3), dtype=torch.float64, device=device).index_add_(0, cluster, p64) / members[:, None]
  a, b, c = p64[index[:, 0]], p64[index[:, 1]], p64[index[:, 2]]
  m = torch.linalg.cross(b - a, c - a)
  outer = (m[:, :, None] * m[:, None, :]).reshape(-1, 9)
  A = torch.zeros((count, 9), dtype=torch.float64, device=device)
  r = torch.zeros((count, 3), dtype=torch.float64, device=device)
  for k in range(3):
    corner = cluster[index[:, k]]
    d = -(m * (a - mean[corner])).sum(dim=1)
    A.index_add_(0, corner, outer)
    r.index_add_(0, corner, d[:, None] * m)
  A = A.reshape(count, 3, 3)
  trace = A.diagonal(dim1=1, dim2=2).sum(dim=1)
  solvable = trace > 0
  eye = torch.eye(3, dtype=torch.float64, device=device)
  M = torch.where(solvable[:, None, None], A + (regularisation * trace / 3.0)[:, None, None] * eye, eye)
  x = (mean - torch.linalg.solve(M, r)).float()
  cluster_cell = torch.stack([unique_keys & (2 ** 21 - 1), (unique_keys >> 21) & (2 ** 21 - 1), (unique_keys >> 42) & (2 ** 21 - 1)], dim=1)
  inside = lambda p: (torch.floor((p - origin) / size).long() == cluster_cell).all(dim=1)
  first = torch.full((count,), vertices.shape[0], dtype=torch.long, device=device).scatter_reduce(
    0, cluster, torch.arange(vertices.shape[0], device=device), 'amin')
  mean32 = mean.float()
  position = torch.where((solvable & inside(x))[:, None], x,
                         torch.where(inside(mean32)[:, None], mean32, vertices[first.clamp(max=vertices.shape[0] - 1)]))
  triple = cluster[index]
  alive = (triple[:, 0] != triple[:, 1]) & (triple[:, 1] != triple[:, 2]) & (triple[:, 2] != triple[:, 0])
  triple = triple[alive]
  shift = triple.argmin(dim=1)
  triple = torch.gather(triple, 1, (shift[:, None] + torch.arange(3, device=device)) % 3)
  assert count < 2 ** 21
  packed = (triple[:, 0] << 42) | (triple[:, 1] << 21) | triple[:, 2]
  _, which = torch.unique(packed, return_inverse=True)
  lowest = torch.full((int(which.max()) + 1 if which.numel() else 0,), packed.shape[0], dtype=torch.long, device=device).scatter_reduce(
    0, which, torch.arange(packed.shape[0], device=device), 'amin')
  triple = triple[lowest.sort().values]
  used, new_faces = torch.unique(triple, return_inverse=True)
  return position[used], new_faces.to(torch.int32)


def main():
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--volume', type=int, default=512)
  p.add_argument('--rounds', type=int, default=5)
  p.add_argument('--warmup', type=int, default=2)
  p.add_argument('--lattice', type=int, default=30, help="spacing, in samples, of the lattice of one-cell shells")
  p.add_argument('--cells', type=float, nargs='+', default=[2.0, 4.0, 8.0], help="cell sizes in voxels")
  args = p.parse_args()
  if not torch.cuda.is_available():
    sys.exit("bench_mesh_simplify: no GPU visible (there is no CPU fallback to time)")
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
  mesh = volume.extract_mesh()
  del volume
  torch.cuda.synchronize()
  num_vertices, num_faces = mesh.vertices.shape[0], mesh.faces.shape[0]
  stream_bytes = 12 * num_vertices + 12 * num_faces
  read_ms = stream_bytes / COPY_RATE * 1e3
  print(f"== {n}^3 sphere + {int(free.sum())} one-cell shells: {num_vertices} vertices, {num_faces} triangles; one streaming read "
        f"of vertices and faces ({stream_bytes / 1e6:.1f} MB): {read_ms:.4f} ms at {COPY_RATE / 1e12:.1f} TB/s")
  src = torch.empty((stream_bytes // 4,), dtype=torch.float32, device=device)
  dst = torch.empty_like(src)

  for cells in args.cells:
    cell_size = cells * voxel
    got, vertex_map, origin, choice, cluster_scan = tm._simplify(mesh, cell_size, None, 'quadric', 1e-3)
    kept = cluster_scan[1:] != cluster_scan[:-1]                        # the clusters that still have a face
    clusters = int(kept.shape[0])
    took = torch.bincount(choice[kept].long(), minlength=3).tolist()
    print(f"== cell of {cells:g} voxels: {clusters} clusters -> {got.vertices.shape[0]} vertices, {got.faces.shape[0]} triangles "
          f"({num_faces / max(got.faces.shape[0], 1):.1f} x fewer); positions taken: quadric {took[0]}, mean {took[1]}, member {took[2]}")
    again = tm.simplify_mesh(mesh, cell_size)
    assert torch.equal(again.vertices.view(torch.int32), got.vertices.view(torch.int32)) and torch.equal(again.faces, got.faces)
    composed_vertices, composed_faces = torch_simplify(mesh.vertices, mesh.faces, origin, cell_size)
    same = composed_vertices.shape == got.vertices.shape and torch.equal(composed_faces, got.faces)
    print(f"   torch composition: {composed_vertices.shape[0]} vertices, {composed_faces.shape[0]} triangles; "
          f"{'faces equal the kernels' if same else 'FACES DIFFER'}"
          + (f"; largest position difference {float((composed_vertices - got.vertices).abs().max()):.3e}" if same else ""))
    del composed_vertices, composed_faces, again
    variants = {
      "simplify_mesh(placement='quadric')": lambda: tm.simplify_mesh(mesh, cell_size),
      "simplify_mesh(placement='mean')": lambda: tm.simplify_mesh(mesh, cell_size, placement='mean'),
      'torch: unique + index_add_ + linalg.solve': lambda: torch_simplify(mesh.vertices, mesh.faces, origin, cell_size),
      'device copy of vertices + faces bytes': lambda: dst.copy_(src),
    }
    median = interleaved(variants, args.rounds, args.warmup)
    whole, other = median["simplify_mesh(placement='quadric')"], median['torch: unique + index_add_ + linalg.solve']
    print(f"   simplify_mesh {whole:.3f} ms = {whole / read_ms:.1f} x one streaming read; torch composition {other:.3f} ms = "
          f"{other / whole:.2f} x the call ({'call faster' if other > whole else 'CALL SLOWER'})")
    print("   stage by stage (medians; the host read is the wait for the stages before it):")
    stages = staged(mesh, cell_size, 'quadric', args.rounds, args.warmup)
    for name, ms in stages:
      print(f"     {name:40s} {ms:9.3f} ms")
    gather_bytes = 3 * num_faces * (4 + 12 + 36) + num_vertices * (4 + 12)      # every vertex of an extracted mesh is referenced
    gather_ms = gather_bytes / COPY_RATE * 1e3
    placement = dict(stages)['placement']
    print(f"   placement kernel: {3 * num_faces} corners, {gather_bytes / 1e6:.1f} MB named by its gathers = {gather_ms:.4f} ms at "
          f"{COPY_RATE / 1e12:.1f} TB/s; measured {placement:.3f} ms = {placement / gather_ms:.1f} x that")


if __name__ == '__main__':
  main()
