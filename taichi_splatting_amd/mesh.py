"""Mesh clean-up on the GPU (``csrc/mesh.hip``): connected components of a ``TriangleMesh`` (``mesh_components``), face
selection with vertex compaction (``select_faces``), removal of small components (``remove_small_components`` — the
floater removal 2DGS, GOF and PGSR apply to an extracted mesh) and area-weighted vertex normals (``vertex_normals``,
``with_vertex_normals``).  These close the mesh path: ``extract_mesh`` -> label -> drop -> shade -> ``save_mesh_ply``.

``vertices`` float32 ``(V, 3)`` and ``faces`` int32 ``(T, 3)``, contiguous, on the GPU; a CPU tensor raises (there is no
CPU fallback).  ``V <= 2^31 - 1`` and ``3 T <= 2^31 - 1``.  Every call accepts ``T = 0``, ``V = 0``, degenerate faces
(``a == b``), duplicate faces and vertices no face references.  Faces are connected through shared vertex indices only,
never through coinciding positions.  Two runs of any call return bitwise-equal tensors.  The label rule, the selection
order and the normal formula are stated in ``include/mi355_splat.h``; ``tests/mesh_oracle.py`` holds them in numpy.

Out of scope: simplification or decimation, hole filling, smoothing, welding vertices by position, non-manifold repair,
per-component areas, float64 meshes, gradients and more than one GPU.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
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
  return TriangleMesh(vertices=out_vertices, faces=out_faces, colours=out_colours, normals=out_normals)


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


__all__ = ["MeshComponents", "mesh_components", "select_faces", "remove_small_components", "vertex_normals",
           "vertex_normal_sums", "with_vertex_normals", "MAX_VERTICES", "MAX_CORNERS"]
