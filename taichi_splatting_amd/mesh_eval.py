"""How good is a mesh?  Surface samples of a ``TriangleMesh`` (``csrc/mesh_sample.hip``), nearest neighbours between two
point sets (``misc.knn_query``, ``csrc/knn_query.hip``) and the two reductions every mesh-from-splats paper reports:
Chamfer distance (DTU: 2DGS, GOF, PGSR) and precision / recall / F-score at a threshold (Tanks and Temples).  This closes
the mesh path with a number: ``extract_mesh`` -> ``remove_small_components`` -> ``simplify_mesh`` -> ``evaluate_mesh``.

Samples are uniform over the surface, area-weighted and STRATIFIED: sample ``i`` of ``n`` falls into the ``i``-th of ``n``
equal shares of the cumulative face area, so a face of area ``a`` receives ``n a / A`` samples to within 2, and a face of
zero area none.  They are seeded by a counter-based generator — a function of ``(seed, i)`` and of no state — so two calls
return the same bits.  The formulas, the generator included, are stated in ``include/mi355_splat.h``;
``tests/mesh_sample_oracle.py`` holds them in numpy.

Distances are between POINT SETS, as the benchmarks' own evaluation scripts measure them: the mesh is sampled densely and
each sample finds its nearest reference point, each reference point its nearest sample.  Out of scope: exact
point-to-triangle distance, gradients, visibility masks and observation volumes of specific datasets (a caller crops both
clouds first), more than one GPU.
"""
from __future__ import annotations

from dataclasses import dataclass
import math
import numbers
import operator
from typing import Optional, Tuple

import torch

from . import _lib
from .fusion import TriangleMesh
from .mesh import _check_mesh, _status
from .misc.knn import knn_query


@dataclass
class SurfaceSamples:
  """``points`` (n, 3) float32; ``colours`` / ``normals`` (n, 3) float32 or None (interpolated from the vertex rows when
  the mesh has them; normals are not renormalised; ``face_normals=True`` gives the unit face normal instead); ``faces``
  (n,) int32 and ``barycentric`` (n, 3) float32 when asked for."""
  points: torch.Tensor
  colours: Optional[torch.Tensor] = None
  normals: Optional[torch.Tensor] = None
  faces: Optional[torch.Tensor] = None
  barycentric: Optional[torch.Tensor] = None


@dataclass(frozen=True)
class SurfaceMetrics:
  """``accuracy`` = mean distance from a point of A to its nearest point of B, ``completeness`` = the mean the other way
  round, ``chamfer`` = their mean (the DTU convention); ``precision`` / ``recall`` = the share of A / B within the
  threshold, ``fscore`` their harmonic mean (0 when both are 0); ``dropped_a`` / ``dropped_b`` = the share of distances
  above ``max_distance`` that were left out of the two means (0 without one)."""
  accuracy: float
  completeness: float
  chamfer: float
  precision: float
  recall: float
  fscore: float
  dropped_a: float
  dropped_b: float


def _face_areas(mesh: TriangleMesh, what: str) -> Tuple[torch.Tensor, torch.Tensor]:
  """((T,) float64 areas, (1,) int32 status) on the device: no host read"""
  vertices, faces, num_vertices, num_faces = _check_mesh(mesh, what)
  device = vertices.device
  area = torch.empty((num_faces,), dtype=torch.float64, device=device)
  status = torch.empty((1,), dtype=torch.int32, device=device)
  _lib.check(_lib.load().ms_mesh_face_areas(vertices.data_ptr(), faces.data_ptr(), num_vertices, num_faces, area.data_ptr(),
                                            status.data_ptr(), _lib.current_stream(device)), what)
  return area, status


def _area_status(status: int, what: str, num_vertices: int):
  _status(status, what, num_vertices)
  if status & _lib.MESH_NOT_FINITE:
    raise ValueError(f"{what}: a vertex that a face references is not finite")


def face_area_cdf(mesh: TriangleMesh) -> torch.Tensor:
  """(T,) float64 inclusive cumulative sum of the face areas ``0.5 |(b - a) x (c - a)|`` (float64 on the float32
  positions), the last entry being the surface area.  A face with an index outside ``0 .. V - 1`` or a vertex that is
  not finite counts as area 0 here (this call has no host read); ``sample_mesh_points`` raises for it."""
  return torch.cumsum(_face_areas(mesh, "face_area_cdf")[0], dim=0)


def _sample_count(n, density, area: Optional[float]) -> Optional[int]:
  """n as an integer >= 1; None while it still depends on the area"""
  if (n is None) == (density is None):
    raise ValueError("sample_mesh_points: exactly one of n and density is expected")
  if n is not None:
    if isinstance(n, bool):
      raise ValueError(f"sample_mesh_points: n must be a positive integer (got {n!r})")
    try:
      n = operator.index(n)
    except TypeError:
      raise ValueError(f"sample_mesh_points: n must be a positive integer (got {n!r})") from None
  else:
    if isinstance(density, bool) or not isinstance(density, numbers.Real) or not math.isfinite(density) or density <= 0:
      raise ValueError(f"sample_mesh_points: density must be a finite positive number of samples per unit area (got {density!r})")
    if area is None:
      return None
    n = math.ceil(float(density) * area)
  if n < 1:
    raise ValueError(f"sample_mesh_points: n >= 1 expected (got {n})")
  if n >= 2 ** 31:
    raise ValueError(f"sample_mesh_points: n < 2^31 expected (got {n})")
  return n


def sample_mesh_points(mesh: TriangleMesh, n: Optional[int] = None, *, density: Optional[float] = None, seed: int = 0,
                       return_faces: bool = False, return_barycentric: bool = False,
                       face_normals: bool = False) -> SurfaceSamples:
  """``n`` points (or ``ceil(density x area)``: exactly one of the two is given) uniformly on the surface of ``mesh``,
  area-weighted, stratified over the cumulative face area and seeded: the same ``(mesh, n, seed)`` gives the same bits.
  ``colours`` and ``normals`` of the mesh are interpolated with the samples' barycentric weights;
  ``face_normals=True`` returns the unit normal of the drawn face instead (and needs no vertex normals).
  ``return_faces`` / ``return_barycentric`` add the face index and the weights ``(wa, wb, wc)`` of every sample.

  Areas, a cumulative sum, ONE host read (the total area and the status word), one launch.  ``ValueError`` for a mesh
  without faces or of zero (or non-finite) total area, a face index outside ``0 .. V - 1``, a referenced vertex that is
  not finite, ``n < 1``, and for both or neither of ``n`` and ``density``."""
  what = "sample_mesh_points"
  count = _sample_count(n, density, None)
  if not isinstance(seed, int) or isinstance(seed, bool):
    raise ValueError(f"{what}: seed must be an integer (got {seed!r})")
  vertices, faces, num_vertices, num_faces = _check_mesh(mesh, what)
  if num_faces == 0:
    raise ValueError(f"{what}: the mesh has no faces")
  device = vertices.device
  area, status = _face_areas(mesh, what)
  cdf = torch.cumsum(area, dim=0)
  total, bits = torch.cat([cdf[-1:], status.to(torch.float64)]).cpu().tolist()        # the one host read
  _area_status(int(bits), what, num_vertices)
  if not (math.isfinite(total) and total > 0.0):
    raise ValueError(f"{what}: the total area of the mesh is {total}: nothing to sample")
  if count is None:
    count = _sample_count(None, density, total)

  f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
  colours = None if mesh.colours is None else mesh.colours.detach()
  normals = None if mesh.normals is None or face_normals else mesh.normals.detach()
  out = SurfaceSamples(points=f32(count, 3),
                       colours=None if colours is None else f32(count, 3),
                       normals=f32(count, 3) if (normals is not None or face_normals) else None,
                       faces=torch.empty((count,), dtype=torch.int32, device=device) if return_faces else None,
                       barycentric=f32(count, 3) if return_barycentric else None)
  _lib.check(_lib.load().ms_mesh_sample_points(
    vertices.data_ptr(), faces.data_ptr(), _lib.ptr(colours), _lib.ptr(normals), num_vertices, num_faces, cdf.data_ptr(),
    count, seed & 0xffffffff, out.points.data_ptr(), _lib.ptr(out.faces), _lib.ptr(out.barycentric), _lib.ptr(out.colours),
    _lib.ptr(out.normals), _lib.current_stream(device)), what)
  return out


def _check_cloud(points, name: str, what: str) -> torch.Tensor:
  if not isinstance(points, torch.Tensor) or points.ndim != 2 or points.shape[1] != 3:
    raise ValueError(f"{what}: {name} must be a (N, 3) tensor, got {tuple(getattr(points, 'shape', ()))}")
  if points.shape[0] == 0:
    raise ValueError(f"{what}: {name} is empty")
  return points


def surface_distances(a_points: torch.Tensor, b_points: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
  """(d_ab (Na,), d_ba (Nb,)) float32: the distance from every point of A to its nearest point of B, and the other way
  round — the float32 square root of ``knn_query(..., k=1)`` in both directions.  Both sets non-empty, finite, on one
  GPU."""
  what = "surface_distances"
  a, b = _check_cloud(a_points, 'a_points', what), _check_cloud(b_points, 'b_points', what)
  d_ab = knn_query(a, b, 1, return_indices=False)[0]
  d_ba = knn_query(b, a, 1, return_indices=False)[0]
  return torch.sqrt(d_ab[:, 0]), torch.sqrt(d_ba[:, 0])


def _check_threshold(threshold, max_distance, what: str):
  for name, v, optional in (('threshold', threshold, False), ('max_distance', max_distance, True)):
    if v is None and optional:
      continue
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or math.isnan(v) or v < 0:
      raise ValueError(f"{what}: {name} must be a number >= 0 (got {v!r})")


def metrics_from_distances(d_ab: torch.Tensor, d_ba: torch.Tensor, threshold: float,
                           max_distance: Optional[float] = None) -> SurfaceMetrics:
  """``SurfaceMetrics`` of the two distance sets of ``surface_distances``: float64 ``torch.sum`` reductions on the
  tensors' device, one host read.  With ``max_distance`` the distances above it are left out of the two MEANS (the DTU
  outlier cap) and their shares reported; precision and recall always count every distance.  A mean over nothing (every
  distance dropped) is NaN."""
  what = "surface_metrics"
  _check_threshold(threshold, max_distance, what)
  row = []
  for name, d in (('d_ab', d_ab), ('d_ba', d_ba)):
    if not isinstance(d, torch.Tensor) or d.ndim != 1 or d.shape[0] == 0:
      raise ValueError(f"{what}: {name} must be a non-empty (N,) tensor, got {tuple(getattr(d, 'shape', ()))}")
    d64 = d.detach().to(torch.float64)
    kept = torch.ones_like(d64, dtype=torch.bool) if max_distance is None else d64 <= float(max_distance)
    row += [torch.sum(torch.where(kept, d64, torch.zeros_like(d64))), torch.sum(kept.to(torch.float64)),
            torch.sum((d64 <= float(threshold)).to(torch.float64))]
  sum_a, kept_a, within_a, sum_b, kept_b, within_b = torch.stack(row).cpu().tolist()       # the one host read
  na, nb = d_ab.shape[0], d_ba.shape[0]
  accuracy = sum_a / kept_a if kept_a > 0 else math.nan
  completeness = sum_b / kept_b if kept_b > 0 else math.nan
  precision, recall = within_a / na, within_b / nb
  fscore = 2.0 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
  return SurfaceMetrics(accuracy=accuracy, completeness=completeness, chamfer=(accuracy + completeness) / 2.0,
                        precision=precision, recall=recall, fscore=fscore, dropped_a=(na - kept_a) / na,
                        dropped_b=(nb - kept_b) / nb)


def surface_metrics(a_points: torch.Tensor, b_points: torch.Tensor, threshold: float,
                    max_distance: Optional[float] = None) -> SurfaceMetrics:
  """Accuracy, completeness, Chamfer distance, precision, recall and F-score of the point set A (samples of a
  reconstruction) against B (the reference): ``surface_distances`` + ``metrics_from_distances``."""
  _check_threshold(threshold, max_distance, "surface_metrics")
  return metrics_from_distances(*surface_distances(a_points, b_points), threshold, max_distance)


def evaluate_mesh(mesh: TriangleMesh, reference_points: torch.Tensor, threshold: float, *, n: Optional[int] = None,
                  density: Optional[float] = None, seed: int = 0, max_distance: Optional[float] = None) -> SurfaceMetrics:
  """``surface_metrics(sample_mesh_points(mesh, n, density=density, seed=seed).points, reference_points, threshold,
  max_distance)``: the mesh is A, the reference cloud B."""
  _check_threshold(threshold, max_distance, "evaluate_mesh")
  _check_cloud(reference_points, 'reference_points', "evaluate_mesh")
  samples = sample_mesh_points(mesh, n, density=density, seed=seed)
  return surface_metrics(samples.points, reference_points, threshold, max_distance)


__all__ = ["SurfaceSamples", "SurfaceMetrics", "face_area_cdf", "sample_mesh_points", "surface_distances",
           "surface_metrics", "metrics_from_distances", "evaluate_mesh"]
