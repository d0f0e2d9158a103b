"""Mesh clean-up on the GPU (``csrc/mesh.hip``): connected components of a ``TriangleMesh`` (``mesh_components``), face
selection with vertex compaction (``select_faces``), removal of small components (``remove_small_components`` — the
floater removal 2DGS, GOF and PGSR apply to an extracted mesh) and area-weighted vertex normals (``vertex_normals``,
``with_vertex_normals``), and simplification by vertex clustering with a quadric-error representative per grid cell
(``simplify_mesh``, ``csrc/mesh_simplify.hip``).  These close the mesh path: ``extract_mesh`` -> label -> drop ->
simplify -> shade -> ``save_mesh_ply``.

``vertices`` float32 ``(V, 3)`` and ``faces`` int32 ``(T, 3)``, contiguous, on the GPU; a CPU tensor raises (there is no
CPU fallback).  ``V <= 2^31 - 1`` and ``3 T <= 2^31 - 1``.  Every call accepts ``T = 0``, ``V = 0``, degenerate faces
(``a == b``), duplicate faces and vertices no face references.  Faces are connected through shared vertex indices only,
never through coinciding positions.  Two runs of any call return bitwise-equal tensors.  The label rule, the selection
order, the normal formula and the four rules of the simplification are stated in ``include/mi355_splat.h``;
``tests/mesh_oracle.py`` and ``tests/mesh_simplify_oracle.py`` hold them in numpy.

Out of scope: edge-collapse decimation to a target face count, hole filling, smoothing, welding vertices by position, non-manifold repair,
per-component areas, float64 meshes, gradients and more than one GPU.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, replace
import math
import numbers
import operator
from typing import Optional, Tuple, Union

import torch

from . import _lib
from .fusion import TriangleMesh

MAX_VERTICES = _lib.MESH_MAX_VERTICES
MAX_CORNERS = _lib.MESH_MAX_CORNERS


@dataclass
class MeshComponents:
  """``vertex_label`` (V,) int32 and ``face_label`` (T,) int32: dense labels ``0 .. K - 1`` ordered by the smallest vertex
  index of the component, ``-1`` for a vertex no face references; ``num_components`` = K; ``face_count`` and
  ``vertex_count`` (K,) int32."""
  vertex_label: torch.Tensor
  face_label: torch.Tensor
  num_components: int
  face_count: torch.Tensor
  vertex_count: torch.Tensor


def _check_mesh(mesh, what: str) -> Tuple[torch.Tensor, torch.Tensor, int, int]:
  """argument errors, before any device work"""
  if not isinstance(mesh, TriangleMesh):
    raise TypeError(f"{what} expects a TriangleMesh (got {type(mesh).__name__})")
  vertices, faces = mesh.vertices, mesh.faces
  optional = [('colours', mesh.colours), ('normals', mesh.normals)]
  for name, t in [('vertices', vertices), ('faces', faces)] + [(n, t) for n, t in optional if t is not None]:
    if not isinstance(t, torch.Tensor):
      raise TypeError(f"{what}: mesh.{name} must be a tensor (got {type(t).__name__})")
  if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
    raise ValueError(f"{what}: vertices (V, 3) and faces (T, 3) expected (got {tuple(vertices.shape)}, {tuple(faces.shape)})")
  if vertices.dtype != torch.float32 or faces.dtype != torch.int32:
    raise TypeError(f"{what}: float32 vertices and int32 faces expected (got {vertices.dtype}, {faces.dtype})")
  num_vertices, num_faces = vertices.shape[0], faces.shape[0]
  if num_vertices > MAX_VERTICES or 3 * num_faces > MAX_CORNERS:
    raise ValueError(f"{what}: V <= 2^31 - 1 and 3 T <= 2^31 - 1 expected (got V = {num_vertices}, T = {num_faces})")
  for name, t in optional:
    if t is not None and (tuple(t.shape) != (num_vertices, 3) or t.dtype != torch.float32):
      raise ValueError(f"{what}: mesh.{name} must be float32 (V, 3) = ({num_vertices}, 3) (got {t.dtype} {tuple(t.shape)})")
  _lib.require_gpu(vertices, faces, mesh.colours, mesh.normals)
  for name, t in [('vertices', vertices), ('faces', faces)] + optional:
    if t is not None and (not t.is_contiguous() or t.device != vertices.device):
      raise ValueError(f"{what}: mesh.{name} must be contiguous and on {vertices.device}")
  return vertices.detach(), faces.detach(), num_vertices, num_faces


def _status(status: int, what: str, num_vertices: int):
  if status < 0:
    raise RuntimeError(f"{what}: the device never reported back (the status word still holds its poison value {status})")
  if status & _lib.MESH_BAD_INDEX:
    raise ValueError(f"{what}: a face refers to a vertex outside 0..{num_vertices - 1}")
  if status & _lib.MESH_GAVE_UP:
    raise RuntimeError(f"{what}: a lane of the union-find exhausted its retries; the labels are not valid")


def _positive_int(value, name: str) -> int:
  if isinstance(value, bool):
    raise ValueError(f"{name} must be a positive integer (got {value!r})")
  try:
    value = operator.index(value)
  except TypeError:
    raise ValueError(f"{name} must be a positive integer (got {value!r})") from None
  if value < 1:
    raise ValueError(f"{name} >= 1 expected (got {value})")
  return min(value, 2 ** 62)


def mesh_components(mesh: TriangleMesh) -> MeshComponents:
  """Connected components of the faces' vertex graph: two vertices belong to one component iff a chain of faces links
  them.  Labels are dense, ``0 .. K - 1``, ordered by the smallest vertex index in the component — so the result does not
  depend on launch order or on any permutation of the face list.  A vertex no face references gets ``-1``, belongs to no
  component and is not counted.

  Lock-free union-find (init, hook, flatten), one exclusive scan of the root flags, labels by gather; then ONE host read,
  of ``K`` and the status word — a face index outside ``0 .. V - 1`` is found on the device (nothing is read or written
  through it) and raises ``ValueError`` here, with the mesh untouched — and one launch per count array."""
  vertices, faces, num_vertices, num_faces = _check_mesh(mesh, "mesh_components")
  device = vertices.device
  lib, stream = _lib.load(), _lib.current_stream(device)
  vertex_label = torch.empty((num_vertices,), dtype=torch.int32, device=device)
  face_label = torch.empty((num_faces,), dtype=torch.int32, device=device)
  head = torch.empty((2,), dtype=torch.int32, device=device)
  call = lambda tmp, size: lib.ms_mesh_components(faces.data_ptr(), num_vertices, num_faces, vertex_label.data_ptr(),
                                                  face_label.data_ptr(), head.data_ptr(), tmp, size, stream)
  _lib.run_with_scratch(call, device, "mesh_components")
  count, status = (int(x) for x in head.cpu())                       # the one host read: K and the status word
  _status(status, "mesh_components", num_vertices)
  vertex_count = torch.empty((count,), dtype=torch.int32, device=device)
  face_count = torch.empty((count,), dtype=torch.int32, device=device)
  _lib.check(lib.ms_mesh_component_counts(vertex_label.data_ptr(), num_vertices, face_label.data_ptr(), num_faces, count,
                                          vertex_count.data_ptr(), face_count.data_ptr(), stream), "mesh_components")
  return MeshComponents(vertex_label=vertex_label, face_label=face_label, num_components=count, face_count=face_count,
                        vertex_count=vertex_count)


def select_faces(mesh: TriangleMesh, face_mask: torch.Tensor) -> TriangleMesh:
  """The faces where ``face_mask`` ((T,) bool) is true, the vertices they reference, and remapped indices.  The order of
  surviving vertices and faces is the input's (stable); ``colours`` and ``normals`` are carried along when present; a
  kept row is bit for bit the input row.  An all-false mask gives a legal empty mesh.

  Mark, two exclusive scans, ONE host read (the new ``V`` and ``T``, which size the outputs, and the status word: a kept
  face with an index outside ``0 .. V - 1`` raises ``ValueError``), one gather launch."""
  return _select(mesh, face_mask)[0]


def _select(mesh: TriangleMesh, face_mask: torch.Tensor) -> Tuple[TriangleMesh, torch.Tensor]:
  """``select_faces`` and the ``(V + 1,)`` exclusive scan of its vertex keep flags (``simplify_mesh`` maps through it)"""
  if not isinstance(face_mask, torch.Tensor):
    raise TypeError(f"select_faces: face_mask must be a tensor (got {type(face_mask).__name__})")
  vertices, faces, num_vertices, num_faces = _check_mesh(mesh, "select_faces")
  device = vertices.device
  _lib.require_gpu(face_mask)
  if face_mask.dtype != torch.bool or tuple(face_mask.shape) != (num_faces,):
    raise ValueError(f"select_faces: face_mask must be bool ({num_faces},) (got {face_mask.dtype} {tuple(face_mask.shape)})")
  if face_mask.device != device:
    raise ValueError(f"select_faces: face_mask is on {face_mask.device}, the mesh on {device}")
  mask = face_mask.detach().contiguous().view(torch.uint8)
  lib, stream = _lib.load(), _lib.current_stream(device)
  vertex_scan = torch.empty((num_vertices + 1,), dtype=torch.int32, device=device)
  face_scan = torch.empty((num_faces + 1,), dtype=torch.int32, device=device)
  head = torch.empty((3,), dtype=torch.int32, device=device)
  call = lambda tmp, size: lib.ms_mesh_select_plan(faces.data_ptr(), mask.data_ptr(), num_vertices, num_faces,
                                                   vertex_scan.data_ptr(), face_scan.data_ptr(), head.data_ptr(), tmp, size, stream)
  _lib.run_with_scratch(call, device, "select_faces")
  new_vertices, new_faces, status = (int(x) for x in head.cpu())      # the one host read
  _status(status, "select_faces", num_vertices)
  out_vertices = torch.empty((new_vertices, 3), dtype=torch.float32, device=device)
  out_faces = torch.empty((new_faces, 3), dtype=torch.int32, device=device)
  out_colours = None if mesh.colours is None else torch.empty((new_vertices, 3), dtype=torch.float32, device=device)
  out_normals = None if mesh.normals is None else torch.empty((new_vertices, 3), dtype=torch.float32, device=device)
  if new_vertices > 0 or new_faces > 0:
    _lib.check(lib.ms_mesh_select_gather(
      vertices.data_ptr(), _lib.ptr(None if mesh.colours is None else mesh.colours.detach()),
      _lib.ptr(None if mesh.normals is None else mesh.normals.detach()), faces.data_ptr(), mask.data_ptr(), num_vertices,
      num_faces, vertex_scan.data_ptr(), face_scan.data_ptr(), out_vertices.data_ptr(), _lib.ptr(out_colours),
      _lib.ptr(out_normals), out_faces.data_ptr(), stream), "select_faces")
  return TriangleMesh(vertices=out_vertices, faces=out_faces, colours=out_colours, normals=out_normals), vertex_scan


def remove_small_components(mesh: TriangleMesh, min_faces: int = 1, keep_largest: Optional[int] = None,
                            return_components: bool = False) -> Union[TriangleMesh, Tuple[TriangleMesh, MeshComponents]]:
  """Keep the components with ``face_count >= min_faces``; with ``keep_largest = n`` only the ``n`` largest of those by
  face count, a tie going to the lower label.  ``mesh_components`` + a selection over the ``K`` counts on the device (a
  stable radix sort of ``(-count, label)``) + ``select_faces``: two host reads in all.  ``return_components=True`` also
  returns the ``MeshComponents`` of the INPUT mesh.  ``ValueError`` for ``min_faces < 1``, ``keep_largest < 1`` or a
  non-integer."""
  min_faces = _positive_int(min_faces, 'min_faces')
  keep_largest = 0 if keep_largest is None else _positive_int(keep_largest, 'keep_largest')
  components = mesh_components(mesh)
  device = mesh.vertices.device
  lib, stream = _lib.load(), _lib.current_stream(device)
  num_faces = mesh.faces.shape[0]
  face_mask = torch.empty((num_faces,), dtype=torch.bool, device=device)
  call = lambda tmp, size: lib.ms_mesh_component_filter(
    components.face_count.data_ptr(), components.num_components, min_faces, keep_largest, components.face_label.data_ptr(),
    num_faces, face_mask.data_ptr(), tmp, size, stream)
  _lib.run_with_scratch(call, device, "remove_small_components")
  cleaned = select_faces(mesh, face_mask)
  return (cleaned, components) if return_components else cleaned


def _normals(mesh: TriangleMesh, what: str, sums: bool) -> torch.Tensor:
  vertices, faces, num_vertices, num_faces = _check_mesh(mesh, what)
  device = vertices.device
  lib, stream = _lib.load(), _lib.current_stream(device)
  out = torch.empty((num_vertices, 3), dtype=torch.float32, device=device)
  call = lambda tmp, size: lib.ms_mesh_vertex_normals(vertices.data_ptr(), faces.data_ptr(), num_vertices, num_faces,
                                                      out.data_ptr() if sums else None, None if sums else out.data_ptr(),
                                                      tmp, size, stream)
  _lib.run_with_scratch(call, device, what)
  return out


def vertex_normals(mesh: TriangleMesh) -> torch.Tensor:
  """(V, 3) float32 unit normals: the normalised sum of ``(b - a) x (c - a)`` over a vertex's incident faces — the
  area-weighted normal, oriented as the faces are (outward for ``extract_mesh``).  The sum runs over the vertex's corners
  in ascending corner index ``3 f + k``, in float64 on the float32 positions, and is rounded once.  A vertex whose sum is
  zero, or that no face references, gets ``(0, 0, 0)``, never a NaN.  A face with an index outside ``0 .. V - 1``
  contributes nothing (``mesh_components`` reports such a face; this call cannot: it has no host read).

  No float atomics — the incidence is a stable radix sort of the ``3 T`` (vertex, corner) pairs — and no host read: the
  call captures into a graph once ``V`` and ``T`` are fixed."""
  return _normals(mesh, "vertex_normals", sums=False)


def vertex_normal_sums(mesh: TriangleMesh) -> torch.Tensor:
  """(V, 3) float32: the sum ``vertex_normals`` normalises, rounded to float32 once (twice the vertex's vector area)."""
  return _normals(mesh, "vertex_normal_sums", sums=True)


def with_vertex_normals(mesh: TriangleMesh) -> TriangleMesh:
  """``mesh`` with ``normals`` filled by ``vertex_normals`` (the other tensors shared, not copied)."""
  return replace(mesh, normals=vertex_normals(mesh))


# ---- simplification: vertex clustering with a quadric-error representative (csrc/mesh_simplify.hip) -----------------------

PLACEMENTS = {'quadric': _lib.MESH_SIMPLIFY_QUADRIC, 'mean': _lib.MESH_SIMPLIFY_MEAN}
MAX_CELL = _lib.MESH_SIMPLIFY_MAX_CELL


def _real(value, name: str, what: str) -> float:
  if isinstance(value, bool) or not isinstance(value, numbers.Real):
    raise ValueError(f"simplify_mesh: {name} must be {what} (got {value!r})")
  value = float(value)
  if not math.isfinite(value) or value <= 0.0:
    raise ValueError(f"simplify_mesh: {name} must be {what} (got {value!r})")
  return value


def _simplify_arguments(cell_size, origin, placement, regularisation):
  """argument errors, before any device work: (cell_size as the float32 the CELL RULE divides by, origin as a (3,) tensor
  or a list of 3 floats or None, placement code, regularisation)"""
  cell_size = ctypes.c_float(_real(cell_size, 'cell_size', "a finite positive number")).value        # rounded to float32
  if not math.isfinite(cell_size) or cell_size <= 0.0:
    raise ValueError("simplify_mesh: cell_size must be a finite positive number in float32 as well")
  regularisation = _real(regularisation, 'regularisation', "finite and > 0")
  if not isinstance(placement, str) or placement not in PLACEMENTS:
    raise ValueError(f"simplify_mesh: placement is one of {sorted(PLACEMENTS)} (got {placement!r})")
  if isinstance(origin, torch.Tensor):
    if tuple(origin.shape) != (3,) or origin.is_complex() or origin.dtype == torch.bool:
      raise ValueError(f"simplify_mesh: origin must be (3,) real numbers (got {origin.dtype} {tuple(origin.shape)})")
  elif origin is not None:
    try:
      origin = [float(x) for x in origin]
    except TypeError:
      raise ValueError(f"simplify_mesh: origin must be (3,) real numbers (got {origin!r})") from None
    if len(origin) != 3 or not all(math.isfinite(x) for x in origin):
      raise ValueError(f"simplify_mesh: origin must be (3,) finite numbers (got {origin!r})")
  return cell_size, origin, PLACEMENTS[placement], regularisation


def _simplify_status(status: int, num_vertices: int):
  _status(status, "simplify_mesh", num_vertices)
  if status & _lib.MESH_NOT_FINITE:
    raise ValueError("simplify_mesh: a vertex that a face references is not finite")
  if status & _lib.MESH_CELL_RANGE:
    raise ValueError(f"simplify_mesh: a vertex that a face references falls into a cell outside 0..{MAX_CELL} "
                     "(lower the origin or raise cell_size)")


def _sorted_pairs(keys: torch.Tensor, values: torch.Tensor, key_bytes: int, end_bit: int, what: str):
  """stable ``ms_radix_sort_pairs`` of the (key, int32 value) pairs on the bits ``0 .. end_bit``: new tensors"""
  device, count = keys.device, keys.shape[0]
  keys_sorted, values_sorted = torch.empty_like(keys), torch.empty_like(values)
  lib, stream = _lib.load(), _lib.current_stream(device)
  call = lambda tmp, size: lib.ms_radix_sort_pairs(keys.data_ptr(), values.data_ptr(), keys_sorted.data_ptr(),
                                                   values_sorted.data_ptr(), count, key_bytes, 0, end_bit, tmp, size, stream)
  _lib.run_with_scratch(call, device, what)
  return keys_sorted, values_sorted


def _simplify(mesh: TriangleMesh, cell_size, origin, placement, regularisation, stage=lambda name: None):
  """``simplify_mesh`` with everything it knows: (mesh, vertex_map (V,), origin (3,) on the device, choice (K,) uint8 =
  which position each of the K clusters took: 0 quadric, 1 mean, 2 lowest member, cluster_scan (K + 1,) int32 = the
  selection's exclusive scan over the clusters: cluster c is output vertex cluster_scan[c] iff cluster_scan[c + 1] differs).  ``stage(name)`` is called when a stage has been enqueued
  (tools/bench_mesh_simplify.py records an event there)."""
  what = "simplify_mesh"
  cell_size, origin, placement, regularisation = _simplify_arguments(cell_size, origin, placement, regularisation)
  if isinstance(mesh, TriangleMesh) and any(isinstance(t, torch.Tensor) and not t.is_cuda and t.device.type != 'meta'
                                            for t in (mesh.vertices, mesh.faces, mesh.colours, mesh.normals)):
    raise ValueError("simplify_mesh: the mesh is not on a GPU; taichi_splatting_amd runs on MI355X (gfx950) only and there "
                     "is no CPU fallback")
  vertices, faces, num_vertices, num_faces = _check_mesh(mesh, what)
  device = vertices.device
  colours = None if mesh.colours is None else mesh.colours.detach()
  lib, stream = _lib.load(), _lib.current_stream(device)
  i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=device)

  if origin is None:          # the smallest finite coordinate per axis, on the device: no host read
    origin = torch.empty((3,), dtype=torch.float32, device=device)
    _lib.check(lib.ms_mesh_simplify_origin(vertices.data_ptr(), num_vertices, origin.data_ptr(), stream), what)
  elif isinstance(origin, torch.Tensor):
    origin = origin.detach().to(device=device, dtype=torch.float32).contiguous()
  else:
    origin = torch.tensor(origin, dtype=torch.float32).to(device)
  stage('origin')

  # 1. cell keys of the referenced vertices, sorted: clusters in ascending key order, members in ascending vertex index
  keys = torch.empty((num_vertices,), dtype=torch.int64, device=device)
  values, referenced, status, head = i32(num_vertices), i32(num_vertices), i32(1), i32(2)
  _lib.check(lib.ms_mesh_simplify_keys(vertices.data_ptr(), faces.data_ptr(), num_vertices, num_faces, origin.data_ptr(),
                                       cell_size, referenced.data_ptr(), keys.data_ptr(), values.data_ptr(), status.data_ptr(),
                                       head.data_ptr(), stream), what)
  stage('mark + cell keys')
  sorted_keys, sorted_vertices = _sorted_pairs(keys, values, 8, 64, what)
  stage('sort (key, vertex), 64 bit')
  head_scan = i32(num_vertices + 1)
  _lib.check(lib.ms_mesh_simplify_heads(sorted_keys.data_ptr(), num_vertices, head_scan.data_ptr(), stream), what)
  _lib.exclusive_scan(head_scan.data_ptr(), num_vertices, head_scan.data_ptr(), device, what)
  vertex_cluster, member_begin = i32(num_vertices), i32(num_vertices + 1)
  _lib.check(lib.ms_mesh_simplify_clusters(sorted_keys.data_ptr(), sorted_vertices.data_ptr(), head_scan.data_ptr(), num_vertices,
                                           vertex_cluster.data_ptr(), member_begin.data_ptr(), status.data_ptr(),
                                           head.data_ptr(), stream), what)
  stage('heads + scan + clusters')
  count, bits = (int(x) for x in head.cpu())                          # host read 1 of 2: K and the status word
  stage('host read of (K, status)')
  _simplify_status(bits, num_vertices)

  # 2. the corners of each cluster (the quadric's incidence), as vertex_normals builds a vertex's
  corner_ranges = sorted_corners = None
  if placement == _lib.MESH_SIMPLIFY_QUADRIC and num_faces > 0:
    corner_keys, corner_values = i32(3 * num_faces), i32(3 * num_faces)
    _lib.check(lib.ms_mesh_simplify_corner_keys(faces.data_ptr(), num_vertices, num_faces, vertex_cluster.data_ptr(), count,
                                                corner_keys.data_ptr(), corner_values.data_ptr(), stream), what)
    stage('corner keys')
    corner_keys, sorted_corners = _sorted_pairs(corner_keys, corner_values, 4, max(count.bit_length(), 1), what)
    corner_ranges = i32(max(count, 1), 2)
    _lib.check(lib.ms_find_ranges(corner_keys.data_ptr(), 3 * num_faces, 4, 0, count, corner_ranges.data_ptr(), stream), what)
    stage('sort (cluster, corner) + ranges')

  # 3. one vertex per cluster
  positions = torch.empty((count, 3), dtype=torch.float32, device=device)
  cluster_colours = None if colours is None else torch.empty((count, 3), dtype=torch.float32, device=device)
  choice = torch.empty((count,), dtype=torch.uint8, device=device)
  _lib.check(lib.ms_mesh_simplify_place(
    vertices.data_ptr(), _lib.ptr(colours), faces.data_ptr(), num_vertices, num_faces, origin.data_ptr(), cell_size,
    regularisation, placement, sorted_keys.data_ptr(), sorted_vertices.data_ptr(), member_begin.data_ptr(), count,
    _lib.ptr(corner_ranges), _lib.ptr(sorted_corners), positions.data_ptr(), _lib.ptr(cluster_colours), choice.data_ptr(),
    stream), what)
  stage('placement')

  # 4. the faces over the clusters: collapsed ones dropped, duplicates dropped by two stable sorts
  new_faces, third_keys, face_values = i32(num_faces, 3), i32(num_faces), i32(num_faces)
  keep = torch.empty((num_faces,), dtype=torch.uint8, device=device)
  _lib.check(lib.ms_mesh_simplify_faces(faces.data_ptr(), num_vertices, num_faces, vertex_cluster.data_ptr(), count,
                                        new_faces.data_ptr(), third_keys.data_ptr(), face_values.data_ptr(), keep.data_ptr(),
                                        stream), what)
  stage('rewrite faces')
  if num_faces > 1:
    index_bits = max((count - 1).bit_length(), 1)
    _, order = _sorted_pairs(third_keys, face_values, 4, index_bits, what)
    pair_keys = torch.empty((num_faces,), dtype=torch.int64, device=device)
    _lib.check(lib.ms_mesh_simplify_pair_keys(new_faces.data_ptr(), order.data_ptr(), num_faces, index_bits,
                                              pair_keys.data_ptr(), stream), what)
    _, order = _sorted_pairs(pair_keys, order, 8, 2 * index_bits, what)
    _lib.check(lib.ms_mesh_simplify_dedup(new_faces.data_ptr(), order.data_ptr(), num_faces, keep.data_ptr(), stream), what)
  stage('two sorts + de-duplication')

  # 5. select_faces' compaction drops the clusters no face is left in (host read 2 of 2), and the two maps compose
  clustered = TriangleMesh(vertices=positions, faces=new_faces, colours=cluster_colours)
  simplified, cluster_scan = _select(clustered, keep.view(torch.bool))
  vertex_map = i32(num_vertices)
  _lib.check(lib.ms_mesh_simplify_map(vertex_cluster.data_ptr(), num_vertices, cluster_scan.data_ptr(), count,
                                      vertex_map.data_ptr(), stream), what)
  stage('select_faces + vertex map')
  return simplified, vertex_map, origin, choice, cluster_scan


def simplify_mesh(mesh: TriangleMesh, cell_size: float, origin=None, placement: str = 'quadric', regularisation: float = 1e-3,
                  return_map: bool = False) -> Union[TriangleMesh, Tuple[TriangleMesh, torch.Tensor]]:
  """Vertex clustering (Rossignac & Borrel) on a grid of side ``cell_size`` with Lindstrom's quadric-error representative:
  one output vertex per occupied cell, the faces whose three corners fall into three different cells.  The decimation
  that is a sort, two scans and a per-cluster reduction — deterministic, no float atomics, two runs bitwise equal.  The
  cell, order, face and placement rules are stated in ``include/mi355_splat.h``; ``tests/mesh_simplify_oracle.py`` holds
  them in numpy.

  ``cell(p) = floor((p - origin) / cell_size)`` per axis in float32; ``origin`` is ``(3,)`` (numbers or a tensor) and
  defaults to the smallest finite coordinate of ALL vertices per axis, taken on the device.  Cell indices lie in
  ``0 .. 2^21 - 1``.  Only vertices a face references are clustered.  Output vertices are in ascending cell key
  ``z << 42 | y << 21 | x``, output faces in input order, each rotated so that its smallest index comes first; of equal
  triples the lowest input face survives (opposite orientations are not equal).  ``placement='quadric'`` puts a vertex at
  the minimiser of the summed squared area-weighted distances to the planes of the cluster's faces, pulled towards the
  float64 mean of the members with relative weight ``regularisation``, if that point lies in the cell; else at the mean
  if that does; else at the member with the lowest index.  ``'mean'`` skips the first.  Every output vertex therefore lies in
  its own cell, and simplifying the result again with the same ``origin`` and ``cell_size`` returns the same faces.
  ``colours`` are averaged per cluster; ``normals`` are not carried (``with_vertex_normals`` recomputes them).

  ``return_map=True`` also returns ``vertex_map`` ``(V,)`` int32: the output vertex of every input vertex, ``-1`` for one
  no face references or whose cluster lost all its faces.

  ``ValueError`` before any device work for a ``cell_size`` or ``regularisation`` that is not a finite positive number,
  an unknown ``placement``, an ``origin`` of the wrong shape and a mesh that is not on the GPU; ``ValueError`` after the
  first host read, with the input untouched, for a face index outside ``0 .. V - 1`` and for a referenced vertex that is
  not finite or whose cell index leaves the range (a NaN in an unreferenced vertex is legal).  ``T = 0``, ``V = 0`` and a
  mesh that collapses to nothing are legal.  TWO host reads — the cluster count with the status word, then
  ``select_faces``' — because the output sizes depend on the data: the call does not capture into a graph."""
  simplified, vertex_map = _simplify(mesh, cell_size, origin, placement, regularisation)[:2]
  return (simplified, vertex_map) if return_map else simplified


__all__ = ["MeshComponents", "mesh_components", "select_faces", "remove_small_components", "vertex_normals",
           "vertex_normal_sums", "with_vertex_normals", "simplify_mesh", "MAX_VERTICES", "MAX_CORNERS"]
