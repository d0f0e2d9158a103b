#!/usr/bin/env python
"""Render a 3DGS PLY scene: the door through which a scene that is not synthetic reaches the renderer and its measurements.

Loads the scene onto the GPU (taichi_splatting_amd.scene_io), puts K pinhole cameras (60 degrees across the width) on a
circle around the scene's robust centre — the median position; the circle lies in the x-z plane with +y down, the frame
of a structure-from-motion reconstruction; its radius is 1.2 x the largest 5-95 % extent of the three axes — looking
inwards, and calls render_gaussians(use_sh=True) on each.  Prints ONE JSON line: N, SH degree, the load time split into
read (file -> pinned staging buffer, host seconds) and upload / unpack (device events), and per view the visible
gaussians and tile overlaps; ms per frame is the median over the views after one warm-up pass over all of them.  With
--out the images are written as view_000.npy ... (H, W, 3) float32.

    python tools/render_scene.py scene.ply [--size W H] [--views K] [--out DIR] [--sh-degree d] [--transform "x 90 0.5"]
                                           [--coverage] [--sh-codes K [--coded]]
                                           [--mesh out.ply --voxel-size s [--bounds x0 y0 z0 x1 y1 z1]
                                            [--min-component-faces N] [--keep-components K] [--mesh-cell-size s]
                                            [--mesh-normals]
                                            [--eval-points gt.ply --eval-threshold t [--eval-samples n]]]

--sh-degree d renders SH bands 0..d of the file's degree only (d = 0: the diffuse colours), in place.
--transform "AXIS DEG [SCALE]" (a rotation about x, y or z, then a uniform scale) or 16 numbers (a row-major 4x4
similarity matrix) moves the scene after loading, SH bands included (Gaussians3D.transformed, in place); the cameras
orbit the moved scene.
--coverage runs camera_coverage over the orbit before rendering and adds to the JSON line the time of the call and how
many gaussians are seen by no view, by some but not all (1..K-1), and by all K views (the three counts sum to N).
--sh-codes K vector-quantises the higher SH bands with a K-code k-means codebook (scene_codec.compress_scene, 10 Lloyd
iterations, seed 0), renders the decoded scene beside the original from every view and adds to the JSON line the two
sizes in bytes, the time of the compression and the PSNR between the two renders (peak 1; per view and over all views).
With --out the quantised images are written as quantised_000.npy ....
--mesh out.ply --voxel-size s fuses the depth of the orbit views into a TSDF volume (fusion.fuse_scene: per view
render_gaussians + render_geometry(normals=False), whose F = 2 wide pass dominates the cost — an offline operation) and
writes the marching-tetrahedra mesh as a binary PLY with vertex colours.  --bounds is the volume's box, by default the box
of the gaussians' positions; a box of more than 2^27 samples at that voxel size is refused.  The JSON line gains the
volume's dims, vertex and triangle counts, the times of fusion and extraction, and the median / min / max distance of the
vertices from the orbit centre (for a scene that is a sphere about it, the radial error on record).
--min-component-faces N (default 1: nothing removed) drops the connected components of the mesh with fewer than N
triangles and --keep-components K (default: all) keeps only the K largest (mesh.remove_small_components, on the device);
--mesh-normals adds area-weighted vertex normals (nx ny nz) to the written file.  With either of the first two the JSON
line also gains the counts before cleaning, the number of components found and the time of the clean-up.
--mesh-cell-size s simplifies the mesh by vertex clustering on a grid of side s with quadric placement
(mesh.simplify_mesh, on the device) after the component removal and before --mesh-normals; the JSON line gains the vertex
and triangle counts before and after and the time of the call.
--eval-points gt.ply --eval-threshold t scores the mesh that was just written against a ground-truth point cloud (a PLY
with x y z; scene_io.load_points_ply): --eval-samples n (default 1 000 000) stratified surface samples of the mesh
(mesh_eval.evaluate_mesh, on the device), their nearest ground-truth points and the reverse; the JSON line gains accuracy,
completeness, the Chamfer distance, precision, recall and F-score at the threshold, and the time of the call.
--coded (with --sh-codes) also renders the quantised scene straight from its codebook (render_compressed: no decoded
feature tensor) and adds the PSNR of that render against the decoded one (null when they are identical) and the median
frame time of both, after one warm-up pass each.
"""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from taichi_splatting_amd import CameraParams, RasterConfig, camera_coverage, frame, render_gaussians, scene_io     # noqa: E402
from taichi_splatting_amd.data_types import similarity_from_matrix                                 # noqa: E402


def orbit_cameras(position, views, size, device):
  """``views`` cameras on a circle around the median of ``position`` (N, 3), each looking at it; camera axes x right, y down,
  z forward."""
  w, h = size
  ordered = position.sort(dim=0).values
  n = ordered.shape[0]
  centre = ordered[n // 2]
  extent = float((ordered[min(n - 1, int(0.95 * n))] - ordered[int(0.05 * n)]).max())
  radius = 1.2 * max(extent, 1e-3)
  focal = 0.5 * w / math.tan(math.radians(30.0))
  projection = torch.tensor([focal, focal, 0.5 * w, 0.5 * h], dtype=torch.float32, device=device)
  down = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
  cameras = []
  for v in range(views):
    angle = 2.0 * math.pi * v / views
    eye = centre.double().cpu() + radius * torch.tensor([math.sin(angle), 0.0, -math.cos(angle)], dtype=torch.float64)
    forward = centre.double().cpu() - eye
    forward = forward / forward.norm()
    right = torch.linalg.cross(down, forward)
    right = right / right.norm()
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3] = torch.stack([right, torch.linalg.cross(forward, right), forward])
    T[:3, 3] = -T[:3, :3] @ eye
    cameras.append(CameraParams(projection=projection, T_camera_world=T.to(torch.float32).to(device),
                                near_plane=0.01 * radius, far_plane=100.0 * radius, image_size=(w, h), id=v))
  return cameras, radius


def parse_transform(text):
  """'AXIS DEG [SCALE]' or 16 numbers -> (4, 4) float64; what the matrix may be is Gaussians3D.transformed's to check"""
  tokens = text.replace(',', ' ').split()
  if len(tokens) == 16:
    return torch.tensor([float(x) for x in tokens], dtype=torch.float64).reshape(4, 4)
  if len(tokens) not in (2, 3) or tokens[0].lower() not in ('x', 'y', 'z'):
    raise ValueError(f'--transform expects "AXIS DEG [SCALE]" with AXIS one of x, y, z, or 16 numbers; got {text!r}')
  axis, angle = 'xyz'.index(tokens[0].lower()), math.radians(float(tokens[1]))
  scale = float(tokens[2]) if len(tokens) == 3 else 1.0
  i, j = (axis + 1) % 3, (axis + 2) % 3
  m = torch.eye(4, dtype=torch.float64)
  m[i, i], m[i, j], m[j, i], m[j, j] = math.cos(angle), -math.sin(angle), math.sin(angle), math.cos(angle)
  m[:3, :3] *= scale
  return m


def coverage_report(gaussians, cameras, config):
  """camera_coverage over ``cameras``: ms of the second call (device events; the first warms up) and the histogram of
  views per gaussian in three bins"""
  views = len(cameras)
  with torch.no_grad():
    camera_coverage(gaussians, cameras, config)
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    begin.record()
    cov = camera_coverage(gaussians, cameras, config)
    end.record()
    end.synchronize()
    none, every = int((cov.count == 0).sum()), int((cov.count == views).sum())
  report = dict(views=views, ms=round(begin.elapsed_time(end), 4), seen_by_none=none,
                seen_by_some=cov.count.shape[0] - none - every, seen_by_all=every)
  print(f"coverage: {views} views in {report['ms']:.3f} ms; gaussians seen by 0 / 1..{views - 1} / all {views} views: "
        f"{none} / {report['seen_by_some']} / {every}", file=sys.stderr, flush=True)
  return report


def mesh_report(gaussians, cameras, config, path, voxel_size, bounds, min_component_faces=1, keep_components=None,
                mesh_normals=False, mesh_cell_size=None, eval_points=None, eval_threshold=None, eval_samples=1_000_000):
  """fuse_scene over ``cameras`` + extract_mesh + save_mesh_ply: dims, counts, seconds, vertex distances from the orbit centre"""
  from taichi_splatting_amd import TSDFVolume, fuse_scene, save_mesh_ply
  if bounds is None:
    low, high = gaussians.position.amin(dim=0).tolist(), gaussians.position.amax(dim=0).tolist()
  else:
    low, high = list(bounds[:3]), list(bounds[3:])
  if not all(h >= l for l, h in zip(low, high)):
    raise ValueError(f"--bounds: the upper corner {high} lies below the lower corner {low}")
  dims = tuple(int(math.ceil((h - l) / voxel_size)) + 1 for l, h in zip(low, high))
  volume = TSDFVolume(tuple(low), voxel_size, dims, device=gaussians.position.device)       # ValueError beyond 2^27 samples
  torch.cuda.synchronize()
  start = time.perf_counter()
  fuse_scene(gaussians, cameras, config, volume)
  torch.cuda.synchronize()
  fuse_s = time.perf_counter() - start
  mesh = volume.extract_mesh()
  torch.cuda.synchronize()
  extract_s = time.perf_counter() - start - fuse_s
  cleaning = None
  if min_component_faces > 1 or keep_components is not None:
    from taichi_splatting_amd import remove_small_components
    before = (int(mesh.vertices.shape[0]), int(mesh.faces.shape[0]))
    clean_start = time.perf_counter()
    mesh, components = remove_small_components(mesh, min_faces=min_component_faces, keep_largest=keep_components,
                                               return_components=True)
    torch.cuda.synchronize()
    cleaning = dict(vertices_before=before[0], triangles_before=before[1], components=components.num_components,
                    clean_s=round(time.perf_counter() - clean_start, 4))
  simplification = None
  if mesh_cell_size is not None:
    from taichi_splatting_amd import simplify_mesh
    before = (int(mesh.vertices.shape[0]), int(mesh.faces.shape[0]))
    simplify_start = time.perf_counter()
    mesh = simplify_mesh(mesh, mesh_cell_size)
    torch.cuda.synchronize()
    simplification = dict(cell_size=mesh_cell_size, vertices_before=before[0], triangles_before=before[1],
                          vertices_after=int(mesh.vertices.shape[0]), triangles_after=int(mesh.faces.shape[0]),
                          simplify_s=round(time.perf_counter() - simplify_start, 4))
  if mesh_normals:
    from taichi_splatting_amd import with_vertex_normals
    mesh = with_vertex_normals(mesh)
  save_mesh_ply(mesh, path)
  centre = gaussians.position.sort(dim=0).values[gaussians.position.shape[0] // 2]
  distance = (mesh.vertices - centre).norm(dim=1) if mesh.vertices.shape[0] else torch.zeros((1,), device=centre.device)
  report = dict(path=str(path), dims=list(dims), voxel_size=voxel_size, vertices=int(mesh.vertices.shape[0]),
                triangles=int(mesh.faces.shape[0]), fuse_s=round(fuse_s, 4), extract_s=round(extract_s, 4),
                distance_from_centre=[round(float(x), 6) for x in (distance.median(), distance.min(), distance.max())])
  if cleaning is not None:
    report.update(cleaning)
  if simplification is not None:
    report['simplification'] = simplification
  if mesh_normals:
    report['normals'] = True
  if eval_points is not None:
    from dataclasses import asdict
    from taichi_splatting_amd import evaluate_mesh, load_points_ply
    reference = load_points_ply(eval_points, device=mesh.vertices.device)[0]
    torch.cuda.synchronize()
    eval_start = time.perf_counter()
    metrics = evaluate_mesh(mesh, reference, eval_threshold, n=eval_samples)
    report['evaluation'] = dict(points=str(eval_points), reference_points=int(reference.shape[0]), samples=eval_samples,
                                threshold=eval_threshold, **{k: round(v, 6) for k, v in asdict(metrics).items()},
                                eval_s=round(time.perf_counter() - eval_start, 4))
    print(f"evaluation against {reference.shape[0]} points of {eval_points} with {eval_samples} samples: accuracy "
          f"{metrics.accuracy:.6f}, completeness {metrics.completeness:.6f}, chamfer {metrics.chamfer:.6f}; at {eval_threshold}: "
          f"precision {metrics.precision:.4f}, recall {metrics.recall:.4f}, F-score {metrics.fscore:.4f}", file=sys.stderr, flush=True)
  print(f"mesh: {dims[0]} x {dims[1]} x {dims[2]} samples of {voxel_size}; {report['vertices']} vertices, {report['triangles']} "
        f"triangles -> {path}; fusion of {len(cameras)} views {fuse_s:.3f} s, extraction {extract_s:.3f} s; vertex distance from the "
        f"orbit centre median / min / max {report['distance_from_centre']}", file=sys.stderr, flush=True)
  return report


def timed_frames(render, cameras):
  """median ms per frame of ``render(camera)`` over ``cameras`` after one warm-up pass, and the images of the timed pass"""
  images, frame_ms = [], []
  for camera in cameras:
    render(camera)
  torch.cuda.synchronize()
  for camera in cameras:
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    begin.record()
    image = render(camera)
    end.record()
    end.synchronize()
    frame_ms.append(begin.elapsed_time(end))
    images.append(image)
  return statistics.median(frame_ms), images


def coded_report(scene, decoded, cameras, config, sh_degree):
  """render_compressed beside render_gaussians(decode()): PSNR between the two and both frame times"""
  from taichi_splatting_amd import render_compressed
  with torch.no_grad():
    decoded_ms, decoded_images = timed_frames(lambda cam: render_gaussians(decoded, cam, config, use_sh=True, sh_degree=sh_degree).image, cameras)
    coded_ms, coded_images = timed_frames(lambda cam: render_compressed(scene, cam, config).image, cameras)
  mean = statistics.fmean(float(((a.double() - b.double()) ** 2).mean()) for a, b in zip(coded_images, decoded_images))
  report = dict(coded_psnr_db=round(-10.0 * math.log10(mean), 3) if mean > 0 else None,
                coded_frame_ms=round(coded_ms, 4), decoded_frame_ms=round(decoded_ms, 4))
  print(f"coded: {report['coded_frame_ms']} ms per frame from the codebook, {report['decoded_frame_ms']} ms decoded; PSNR between "
        f"the two {report['coded_psnr_db']} dB", file=sys.stderr, flush=True)
  return report


def quantised_report(gaussians, cameras, config, sh_codes, sh_degree, images, out, coded=False):
  """compress_scene + decode, one render per camera beside ``images`` (the original's): sizes, seconds, PSNR"""
  from taichi_splatting_amd import compress_scene
  torch.cuda.synchronize()
  start = time.perf_counter()
  scene = compress_scene(gaussians, sh_codes=sh_codes, iterations=10, seed=0)
  torch.cuda.synchronize()
  seconds = time.perf_counter() - start
  decoded = scene.decode()
  original_bytes = sum(t.numel() * t.element_size() for t in gaussians.shape_tensors() + (gaussians.feature,))
  squared, per_view = [], []
  with torch.no_grad():
    for v, (camera, image) in enumerate(zip(cameras, images)):
      other = render_gaussians(decoded, camera, config, use_sh=True, sh_degree=sh_degree).image
      mse = float(((other.double() - image.double()) ** 2).mean())
      squared.append(mse)
      per_view.append(round(-10.0 * math.log10(mse), 3) if mse > 0 else None)
      if out:
        np.save(Path(out) / f'quantised_{v:03d}.npy', other.cpu().numpy())
  mean = statistics.fmean(squared)
  report = dict(sh_codes=sh_codes, compress_s=round(seconds, 4), original_bytes=original_bytes, quantised_bytes=scene.nbytes,
                psnr_db=round(-10.0 * math.log10(mean), 3) if mean > 0 else None, psnr_db_per_view=per_view)
  if coded:
    report.update(coded_report(scene, decoded, cameras, config, sh_degree))
  print(f"quantised: {sh_codes} codes in {seconds:.2f} s; {original_bytes} -> {scene.nbytes} bytes "
        f"({original_bytes / scene.nbytes:.2f} x); PSNR between the two renders {report['psnr_db']} dB", file=sys.stderr, flush=True)
  return report


def main():
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('scene')
  p.add_argument('--size', type=int, nargs=2, default=(1024, 768), metavar=('W', 'H'))
  p.add_argument('--views', type=int, default=8)
  p.add_argument('--out', default='')
  p.add_argument('--sh-degree', type=int, default=None, metavar='d',
                 help="active SH degree: render bands 0..d of the file's degree only (default: all of them)")
  p.add_argument('--transform', default=None, metavar='"AXIS DEG [SCALE]"',
                 help="move the loaded scene: a rotation about x, y or z in degrees and a uniform scale, or 16 numbers "
                      "(row-major 4x4 similarity matrix); SH bands are rotated with it")
  p.add_argument('--coverage', action='store_true',
                 help="before rendering, run camera_coverage over the orbit: time, and gaussians seen by 0, 1..K-1, all K views")
  p.add_argument('--sh-codes', type=int, default=None, metavar='K',
                 help="also render the scene with its higher SH bands quantised to a K-code codebook: sizes and PSNR")
  p.add_argument('--coded', action='store_true',
                 help="with --sh-codes: also render straight from the codebook (render_compressed); PSNR against the decoded "
                      "render and both frame times")
  p.add_argument('--mesh', default=None, metavar='out.ply',
                 help="fuse the depth of the orbit views into a TSDF volume and write its mesh (needs --voxel-size)")
  p.add_argument('--voxel-size', type=float, default=None, metavar='s', help="sample spacing of the --mesh volume")
  p.add_argument('--min-component-faces', type=int, default=1, metavar='N',
                 help="drop the connected components of the --mesh mesh with fewer than N triangles (default 1: none)")
  p.add_argument('--keep-components', type=int, default=None, metavar='K',
                 help="keep only the K largest components of the --mesh mesh (default: all)")
  p.add_argument('--mesh-cell-size', type=float, default=None, metavar='s',
                 help="simplify the --mesh mesh by vertex clustering on a grid of side s (default: not simplified)")
  p.add_argument('--mesh-normals', action='store_true', help="write area-weighted vertex normals into the --mesh file")
  p.add_argument('--eval-points', default=None, metavar='gt.ply',
                 help="score the --mesh mesh against this ground-truth point cloud (needs --eval-threshold)")
  p.add_argument('--eval-threshold', type=float, default=None, metavar='t',
                 help="distance within which a point counts for precision / recall / F-score")
  p.add_argument('--eval-samples', type=int, default=1_000_000, metavar='n', help="surface samples of the mesh (default 1 000 000)")
  p.add_argument('--bounds', type=float, nargs=6, default=None, metavar=('x0', 'y0', 'z0', 'x1', 'y1', 'z1'),
                 help="box of the --mesh volume (default: the box of the gaussians' positions)")
  args = p.parse_args()
  if (args.mesh is None) != (args.voxel_size is None) or (args.bounds is not None and args.mesh is None):
    sys.exit("render_scene: --mesh and --voxel-size go together (--bounds is optional with them)")
  if args.mesh is None and (args.min_component_faces != 1 or args.keep_components is not None or args.mesh_normals
                            or args.mesh_cell_size is not None):
    sys.exit("render_scene: --min-component-faces, --keep-components, --mesh-cell-size and --mesh-normals need --mesh")
  if args.min_component_faces < 1 or (args.keep_components is not None and args.keep_components < 1):
    sys.exit("render_scene: --min-component-faces and --keep-components must be at least 1")
  if args.voxel_size is not None and not args.voxel_size > 0:
    sys.exit("render_scene: --voxel-size must be positive")
  if (args.eval_points is None) != (args.eval_threshold is None) or (args.eval_points is not None and args.mesh is None):
    sys.exit("render_scene: --eval-points and --eval-threshold go together, and need --mesh")
  if args.mesh is not None and args.sh_degree is not None:
    sys.exit("render_scene: --mesh fuses the scene with every stored band: it does not combine with --sh-degree")
  if args.coded and args.sh_codes is None:
    sys.exit("render_scene: --coded needs --sh-codes")
  if args.coded and args.sh_degree is not None:
    sys.exit("render_scene: --coded renders every stored band: it does not combine with --sh-degree")
  try:
    transform = parse_transform(args.transform) if args.transform is not None else None
    if transform is not None:
      similarity_from_matrix(transform)             # (refused before the file is read)
  except ValueError as e:
    sys.exit(f"render_scene: --transform: {e}")
  if not torch.cuda.is_available():
    sys.exit("render_scene: no GPU visible (the renderer has no CPU fallback)")
  if args.views < 1:
    sys.exit("render_scene: --views must be at least 1")
  device = torch.device('cuda:0')
  torch.empty(1, device=device)                     # context creation is not load time

  timings = {}
  start = time.perf_counter()
  gaussians = scene_io._load(args.scene, device, 'file', 1 << 20, timings)
  torch.cuda.synchronize()
  load_s = time.perf_counter() - start
  n = gaussians.position.shape[0]
  if n == 0:
    sys.exit(f"render_scene: {args.scene} holds no gaussians")
  degree = math.isqrt(gaussians.feature.shape[2]) - 1
  if args.sh_degree is not None and not 0 <= args.sh_degree <= degree:
    sys.exit(f"render_scene: --sh-degree {args.sh_degree} is outside 0..{degree}, the degree of {args.scene}")
  if transform is not None:
    with torch.no_grad():
      gaussians.transformed(transform, inplace=True)
  cameras, radius = orbit_cameras(gaussians.position, args.views, tuple(args.size), device)
  config = RasterConfig()
  coverage = coverage_report(gaussians, cameras, config) if args.coverage else None

  visible, overlaps, frame_ms, images = [], [], [], []
  with torch.no_grad():
    for camera in cameras:                          # warm-up: every view once (capacities, mapper choice, allocator)
      rendering = render_gaussians(gaussians, camera, config, use_sh=True, sh_degree=args.sh_degree)
      visible.append(int(rendering.points.idx.shape[0]))
      overlaps.append(int(frame.frame_status(rendering)['overlaps']) if hasattr(rendering, 'frame') else None)
    torch.cuda.synchronize()
    for camera in cameras:
      begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      begin.record()
      rendering = render_gaussians(gaussians, camera, config, use_sh=True, sh_degree=args.sh_degree)
      end.record()
      end.synchronize()
      frame_ms.append(begin.elapsed_time(end))
      images.append(rendering.image)
  if args.out:
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    for v, image in enumerate(images):
      np.save(out / f'view_{v:03d}.npy', image.cpu().numpy())
  quantised = None
  if args.sh_codes is not None:
    try:
      quantised = quantised_report(gaussians, cameras, config, args.sh_codes, args.sh_degree, images, args.out, coded=args.coded)
    except ValueError as e:
      sys.exit(f"render_scene: --sh-codes: {e}")
  mesh = None
  if args.mesh is not None:
    try:
      mesh = mesh_report(gaussians, cameras, config, args.mesh, args.voxel_size, args.bounds, args.min_component_faces,
                         args.keep_components, args.mesh_normals, args.mesh_cell_size, args.eval_points, args.eval_threshold,
                         args.eval_samples)
    except ValueError as e:
      sys.exit(f"render_scene: --mesh: {e}")
  print(json.dumps(dict(
    scene=str(args.scene), n=n, sh_degree=degree, sh_active_degree=args.sh_degree, transform=args.transform, image_size=list(args.size), views=args.views, orbit_radius=round(radius, 6),
    load_s=round(load_s, 4), read_s=round(timings['read_s'], 4), upload_ms=round(timings['upload_ms'], 3),
    unpack_ms=round(timings['unpack_ms'], 3), visible=visible, overlaps=overlaps,
    frame_ms=round(statistics.median(frame_ms), 4), frame_ms_per_view=[round(ms, 4) for ms in frame_ms],
    images=str(args.out) if args.out else None, **({'coverage': coverage} if coverage is not None else {}),
    **({'quantised': quantised} if quantised is not None else {}), **({'mesh': mesh} if mesh is not None else {}))), flush=True)


if __name__ == '__main__':
  main()
