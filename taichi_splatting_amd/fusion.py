"""Mesh extraction: fuse depth frames into a truncated signed distance volume (``TSDFVolume.integrate``, one launch of
``ms_tsdf_integrate`` for all frames of a call) and triangulate it (``TSDFVolume.extract_mesh``: marching tetrahedra,
classify -> two scans -> emit), ``csrc/tsdf.hip``.  ``fuse_scene`` renders the depth of a camera set and fuses it;
``save_mesh_ply`` writes the mesh.  The reference has no counterpart: this is the step 2DGS, GOF and PGSR take from
rendered depth to a surface.  ``mesh.py`` cleans the mesh (components, small-part removal) and gives it vertex normals.

float32 only, detached, no autograd; there is no torch fallback and CPU tensors raise, as everywhere in this package.
``integrate`` allocates nothing, never synchronises and never reads back: it captures into a graph.  ``extract_mesh``
reads the two scan totals on the host once, to size its outputs, and therefore does not capture.  No kernel uses an
atomic: both calls are bitwise reproducible.

Out of scope: sparse or hashed volumes, float64, gradients, median depth, marching cubes,
tile-row strips and more than one GPU.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
import math
import operator
import struct
from typing import Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .misc.coverage import CAMERA_VALUES, MAX_CAMERAS, pack_cameras
from .perspective.params import CameraParams

MAX_SAMPLES = _lib.TSDF_MAX_SAMPLES
CAMERA_CHUNK = _lib.TSDF_CAMERA_CHUNK


def _f32(x, name: str) -> float:
  """``x`` rounded to float32 once, as the kernels see it"""
  try:
    value = float(x)
  except (TypeError, ValueError):
    raise TypeError(f"{name} must be a number (got {x!r})") from None
  if math.isnan(value):
    raise ValueError(f"{name} is NaN")
  if math.isinf(value):
    return value
  if abs(value) > 3.4028234663852886e38:
    raise ValueError(f"{name} = {value} does not fit float32")
  return struct.unpack('f', struct.pack('f', value))[0]


@dataclass
class TriangleMesh:
  """``vertices`` (V, 3) float32, ``faces`` (T, 3) int32 (indices into ``vertices``; ``(b - a) x (c - a)`` points to the
  positive, outside, side of the field), ``colours`` (V, 3) float32 or None, ``normals`` (V, 3) float32 or None (filled by
  ``mesh.with_vertex_normals``).  Ordered as ``TSDFVolume.extract_mesh`` states."""
  vertices: torch.Tensor
  faces: torch.Tensor
  colours: Optional[torch.Tensor] = None
  normals: Optional[torch.Tensor] = None


class TSDFVolume:
  """A dense truncated signed distance volume on the GPU.  Samples sit on grid vertices, ``p(i, j, k) = origin +
  voxel_size (i, j, k)``; ``tsdf`` and ``weight`` are ``(nz, ny, nx)`` float32 (x fastest), ``colour`` ``(nz, ny, nx, 3)``
  or None.  Fresh: ``tsdf = 1, weight = 0, colour = 0``.  The tensors are plain attributes: a caller may write a field of
  their own into them (in place; a replacement must keep shape, dtype, device and contiguity).

  ``truncation`` defaults to ``4 voxel_size`` (a default, not a measured choice); ``max_weight=None`` does not clamp the
  weight.  ``ValueError`` before any launch for a dim below 1, more than 2^27 samples (512^3; 2.7 GB with colour: then 7
  possible vertices and 12 possible triangles per cell fit the int32 scans), or a non-positive ``voxel_size``,
  ``truncation`` or ``max_weight``."""

  def __init__(self, origin, voxel_size, dims, truncation=None, colour: bool = True, max_weight=None, device='cuda'):
    try:
      origin = tuple(origin)
      dims = tuple(dims)
    except TypeError:
      raise TypeError(f"origin and dims must be sequences of three numbers (got {origin!r}, {dims!r})") from None
    if len(origin) != 3 or len(dims) != 3:
      raise ValueError(f"origin and dims must have three entries (got {origin!r}, {dims!r})")
    self.origin = tuple(_f32(x, 'origin') for x in origin)
    if any(math.isinf(x) for x in self.origin):
      raise ValueError(f"origin must be finite (got {origin!r})")
    try:
      self.dims = tuple(operator.index(d) for d in dims)
    except TypeError:
      raise TypeError(f"dims must be integers (got {dims!r})") from None
    if any(isinstance(d, bool) for d in dims):
      raise TypeError(f"dims must be integers (got {dims!r})")
    nx, ny, nz = self.dims
    if min(self.dims) < 1 or nx * ny * nz > MAX_SAMPLES:
      raise ValueError(f"every dim >= 1 and nx ny nz <= 2^27 expected (got {self.dims})")
    self.voxel_size = _f32(voxel_size, 'voxel_size')
    if not 0.0 < self.voxel_size < 1e30:
      raise ValueError(f"voxel_size > 0 expected (got {voxel_size})")
    self.truncation = _f32(4.0 * self.voxel_size if truncation is None else truncation, 'truncation')
    if not 0.0 < self.truncation < 1e30:
      raise ValueError(f"truncation > 0 expected (got {truncation})")
    self.max_weight = None if max_weight is None else _f32(max_weight, 'max_weight')
    if self.max_weight is not None and not self.max_weight > 0.0:
      raise ValueError(f"max_weight > 0 (or None: no clamp) expected (got {max_weight})")
    self.device = torch.device(device)
    if self.device.type != 'cuda':
      raise RuntimeError(f"TSDFVolume lives on the GPU (MI355X, gfx950) only: got device {self.device}. There is no CPU fallback.")
    _lib.load()
    self.tsdf = torch.ones((nz, ny, nx), dtype=torch.float32, device=self.device)
    self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=self.device)
    self.colour = torch.zeros((nz, ny, nx, 3), dtype=torch.float32, device=self.device) if colour else None
    self.device = self.tsdf.device
    self._origin_c = (ctypes.c_double * 3)(*self.origin)

  def reset(self) -> 'TSDFVolume':
    """Back to the fresh state, in place."""
    self.tsdf.fill_(1.0)
    self.weight.zero_()
    if self.colour is not None:
      self.colour.zero_()
    return self

  @property
  def num_samples(self) -> int:
    return self.dims[0] * self.dims[1] * self.dims[2]

  def positions(self) -> torch.Tensor:
    """(nz, ny, nx, 3) float32 sample positions, each coordinate as the kernels form it: ``origin + voxel_size * index``."""
    nx, ny, nz = self.dims
    axes = [torch.tensor(self.origin[a], dtype=torch.float32, device=self.device)
            + torch.tensor(self.voxel_size, dtype=torch.float32, device=self.device)
            * torch.arange(n, dtype=torch.float32, device=self.device) for a, n in enumerate((nx, ny, nz))]
    z, y, x = torch.meshgrid(axes[2], axes[1], axes[0], indexing='ij')
    return torch.stack([x, y, z], dim=-1)

  def _fields(self):
    nx, ny, nz = self.dims
    fields = [('tsdf', self.tsdf, (nz, ny, nx)), ('weight', self.weight, (nz, ny, nx))]
    if self.colour is not None:
      fields.append(('colour', self.colour, (nz, ny, nx, 3)))
    for name, t, shape in fields:
      if not isinstance(t, torch.Tensor):
        raise TypeError(f"TSDFVolume.{name} must be a tensor (got {type(t).__name__})")
      _lib.require_gpu(t)
      if tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
        raise ValueError(f"TSDFVolume.{name} must stay a contiguous float32 {shape} tensor on {self.device} "
                         f"(got {t.dtype} {tuple(t.shape)} on {t.device})")
    return self.tsdf, self.weight, self.colour

  # ---- integration ----------------------------------------------------------------------------------------------------

  def _cameras(self, cameras, count: int, width: int, height: int) -> torch.Tensor:
    if isinstance(cameras, CameraParams):
      cameras = [cameras]
    if isinstance(cameras, torch.Tensor):
      if cameras.ndim != 2 or cameras.shape[1] != CAMERA_VALUES:
        raise ValueError(f"packed cameras must be a (C, {CAMERA_VALUES}) tensor (got {tuple(cameras.shape)})")
      _lib.require_gpu(cameras)
      packed = cameras.detach().to(torch.float32).contiguous()
    else:
      try:
        cameras = list(cameras)
      except TypeError:
        raise TypeError("cameras must be a CameraParams, a sequence of them or a packed (C, 20) tensor "
                        f"(got {type(cameras).__name__})") from None
      if not all(isinstance(c, CameraParams) for c in cameras):
        raise TypeError("cameras must be a CameraParams, a sequence of them or a packed (C, 20) tensor")
      if not 1 <= len(cameras) <= MAX_CAMERAS:
        raise ValueError(f"between 1 and {MAX_CAMERAS} cameras expected (got {len(cameras)})")
      for c in cameras:
        if tuple(c.image_size) != (width, height):
          raise ValueError(f"all cameras of a call share the depth images' size (W, H) = ({width}, {height}) "
                           f"(got a camera of {tuple(c.image_size)})")
      _lib.require_gpu(*[t for c in cameras for t in (c.T_camera_world, c.projection)])
      packed = pack_cameras(cameras, torch.float32, self.device)
    if packed.shape[0] != count:
      raise ValueError(f"{count} depth images but {packed.shape[0]} cameras")
    if packed.device != self.device:
      raise ValueError(f"cameras are on {packed.device}, the volume on {self.device}")
    return packed

  def integrate(self, depth: torch.Tensor, cameras: Union[CameraParams, Sequence[CameraParams], torch.Tensor],
                colour: Optional[torch.Tensor] = None, pixel_weight: Optional[torch.Tensor] = None) -> 'TSDFVolume':
    """Fuse ``C`` depth frames, in order, in ONE launch (the rule is stated in ``include/mi355_splat.h``,
    ``ms_tsdf_integrate``; ``tests/tsdf_oracle.py`` holds it in float64).

    ``depth`` ``(C, H, W)`` or ``(H, W)`` float32 camera-z depth, 0 where uncovered — what ``GeometryImages.depth``
    holds; a NaN or an infinity is a hole as well.  ``cameras``: a ``CameraParams``, a sequence of them, or a packed
    ``(C, 20)`` tensor of ``pack_cameras`` (the form for a captured graph); all frames share ``(W, H)``.  ``colour``
    ``(C, H, W, 3)``, required exactly when the volume has colour; ``pixel_weight`` ``(C, H, W)``, a pixel with weight
    <= 0 is skipped.  A sample no frame updates keeps its bits.  ``C`` frames in one call equal ``C`` calls in the same
    order bit for bit; the volume is read and written at most once per call.  Returns ``self``."""
    tsdf, weight, vcolour = self._fields()
    if not isinstance(depth, torch.Tensor):
      raise TypeError(f"depth must be a tensor (got {type(depth).__name__})")
    if depth.dim() == 2:
      depth = depth[None]
      colour = colour[None] if isinstance(colour, torch.Tensor) and colour.dim() == 3 else colour
      pixel_weight = pixel_weight[None] if isinstance(pixel_weight, torch.Tensor) and pixel_weight.dim() == 2 else pixel_weight
    if depth.dim() != 3 or min(depth.shape) < 1:
      raise ValueError(f"depth must be (C, H, W) or (H, W), not empty (got {tuple(depth.shape)})")
    count, height, width = depth.shape
    if height * width >= 2 ** 31:
      raise ValueError(f"image too large {tuple(depth.shape)}")
    if (colour is None) != (vcolour is None):
      raise ValueError("a coloured volume needs colour images and a volume without colour takes none "
                       f"(volume colour: {vcolour is not None}, images: {colour is not None})")
    images = [('depth', depth, (count, height, width))]
    if colour is not None:
      images.append(('colour', colour, (count, height, width, 3)))
    if pixel_weight is not None:
      images.append(('pixel_weight', pixel_weight, (count, height, width)))
    for name, t, shape in images:
      if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor (got {type(t).__name__})")
      if tuple(t.shape) != shape:
        raise ValueError(f"{name} must be {shape} (got {tuple(t.shape)})")
      if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {t.dtype})")
      _lib.require_gpu(t)
      if t.device != self.device:
        raise ValueError(f"{name} is on {t.device}, the volume on {self.device}")
    packed = self._cameras(cameras, count, width, height)
    depth = depth.detach().contiguous()
    colour = None if colour is None else colour.detach().contiguous()
    pixel_weight = None if pixel_weight is None else pixel_weight.detach().contiguous()
    nx, ny, nz = self.dims
    _lib.check(_lib.load().ms_tsdf_integrate(
      tsdf.data_ptr(), weight.data_ptr(), _lib.ptr(vcolour), nx, ny, nz, self._origin_c, self.voxel_size, self.truncation,
      math.inf if self.max_weight is None else self.max_weight, depth.data_ptr(), _lib.ptr(pixel_weight), _lib.ptr(colour),
      packed.data_ptr(), count, width, height, _lib.current_stream(self.device)), "TSDFVolume.integrate")
    return self

  # ---- triangulation --------------------------------------------------------------------------------------------------

  def extract_mesh(self, min_weight: float = 0.0) -> TriangleMesh:
    """Marching tetrahedra on the Kuhn split of every cell into the six corner paths ``(0,0,0) -> (1,1,1)``.

    A sample is valid iff ``weight > 0 and weight >= min_weight`` and inside iff ``tsdf < 0``; a tetrahedron emits
    triangles only when its four corners are valid.  A vertex lies on a grid edge whose ends are valid and differ in
    sign, at ``p_o + l (p_b - p_o)``, ``l = t_o / (t_o - t_b)``, colour with the same ``l``; it is computed once and
    shared by index.  Order (part of the contract): vertices by ``(linear index of the owning lower end o, edge type)``
    with the types ``o -> o + d`` for ``d = 100, 010, 001, 110, 101, 011, 111`` (x, y, z bits); triangles by ``(linear
    index of the cell's lower corner, tetrahedron in lexicographic order of its axis permutation, triangle)``, and
    ``(b - a) x (c - a)`` points to the positive side.  An empty result (``V = T = 0``) is legal.

    Launches: classify, two ``ms_exclusive_scan_i32`` (in place), ONE host read of the two totals to size the outputs —
    so this call synchronises the stream and does not capture into a graph — then emit.  Scratch: 12 bytes per sample.
    No atomics: the result is bitwise reproducible."""
    tsdf, weight, vcolour = self._fields()
    min_weight = _f32(min_weight, 'min_weight')
    lib, stream = _lib.load(), _lib.current_stream(self.device)
    nx, ny, nz = self.dims
    n = nx * ny * nz
    word = torch.empty((n,), dtype=torch.int32, device=self.device)
    vscan = torch.empty((n + 1,), dtype=torch.int32, device=self.device)
    tscan = torch.empty((n + 1,), dtype=torch.int32, device=self.device)
    totals = torch.zeros((2,), dtype=torch.int32).pin_memory()
    _lib.check(lib.ms_tsdf_classify(tsdf.data_ptr(), weight.data_ptr(), nx, ny, nz, min_weight, word.data_ptr(),
                                    vscan.data_ptr(), tscan.data_ptr(), stream), "extract_mesh")
    for slot, scan in enumerate((vscan, tscan)):
      _lib.exclusive_scan(scan.data_ptr(), n, scan.data_ptr(), self.device, "extract_mesh", totals.data_ptr() + 4 * slot)
    torch.cuda.current_stream(self.device).synchronize()          # the one host read: V and T size the outputs
    num_vertices, num_faces = int(totals[0]), int(totals[1])
    vertices = torch.empty((num_vertices, 3), dtype=torch.float32, device=self.device)
    faces = torch.empty((num_faces, 3), dtype=torch.int32, device=self.device)
    colours = None if vcolour is None else torch.empty((num_vertices, 3), dtype=torch.float32, device=self.device)
    if num_vertices > 0:
      faces_ptr = faces.data_ptr() if num_faces > 0 else vertices.data_ptr()       # never written when T = 0
      _lib.check(lib.ms_tsdf_emit(tsdf.data_ptr(), weight.data_ptr(), _lib.ptr(vcolour), nx, ny, nz, self._origin_c,
                                  self.voxel_size, min_weight, word.data_ptr(), vscan.data_ptr(), tscan.data_ptr(),
                                  vertices.data_ptr(), faces_ptr, _lib.ptr(colours), stream), "extract_mesh")
    return TriangleMesh(vertices=vertices, faces=faces, colours=colours)


def save_mesh_ply(mesh: TriangleMesh, path) -> None:
  """Write ``mesh`` as a binary little-endian PLY: element ``vertex`` with float ``x y z`` (+ float ``nx ny nz`` when the
  mesh has normals, + uchar ``red green blue``, ``round(255 clamp(colour, 0, 1))``, when it has colours, in that order),
  element ``face`` with ``list uchar int vertex_indices``.  Tensors on any device."""
  if not isinstance(mesh, TriangleMesh):
    raise TypeError(f"save_mesh_ply expects a TriangleMesh (got {type(mesh).__name__})")
  vertices = mesh.vertices.detach().cpu()
  faces = mesh.faces.detach().cpu()
  if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
    raise ValueError(f"vertices (V, 3) and faces (T, 3) expected (got {tuple(vertices.shape)}, {tuple(faces.shape)})")
  if faces.dtype not in (torch.int32, torch.int64) or not vertices.dtype.is_floating_point:
    raise TypeError(f"float vertices and integer faces expected (got {vertices.dtype}, {faces.dtype})")
  count = vertices.shape[0]
  if faces.numel() and (int(faces.min()) < 0 or int(faces.max()) >= count):
    raise ValueError(f"a face refers to a vertex outside 0..{count - 1}")
  coloured = mesh.colours is not None
  fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
  shaded = mesh.normals is not None
  if shaded:
    normals = mesh.normals.detach().cpu()
    if tuple(normals.shape) != (count, 3) or not normals.dtype.is_floating_point:
      raise ValueError(f"normals must be float (V, 3) = ({count}, 3) (got {normals.dtype} {tuple(normals.shape)})")
    fields += [('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')]
  if coloured:
    colours = mesh.colours.detach().cpu()
    if tuple(colours.shape) != (count, 3):
      raise ValueError(f"colours must be (V, 3) = ({count}, 3) (got {tuple(colours.shape)})")
    fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
  vertex_rows = np.zeros((count,), dtype=np.dtype(fields))
  xyz = vertices.to(torch.float32).numpy()
  for a, name in enumerate('xyz'):
    vertex_rows[name] = xyz[:, a]
  if shaded:
    nxyz = normals.to(torch.float32).numpy()
    for a, name in enumerate(('nx', 'ny', 'nz')):
      vertex_rows[name] = nxyz[:, a]
  if coloured:
    rgb = torch.nan_to_num(colours.to(torch.float32), nan=0.0).clamp(0.0, 1.0).mul(255.0).round().to(torch.uint8).numpy()
    for a, name in enumerate(('red', 'green', 'blue')):
      vertex_rows[name] = rgb[:, a]
  face_rows = np.zeros((faces.shape[0],), dtype=np.dtype([('n', 'u1'), ('v', '<i4', (3,))]))
  face_rows['n'] = 3
  face_rows['v'] = faces.to(torch.int32).numpy()
  header = ["ply", "format binary_little_endian 1.0", f"element vertex {count}",
            "property float x", "property float y", "property float z"]
  if shaded:
    header += ["property float nx", "property float ny", "property float nz"]
  if coloured:
    header += ["property uchar red", "property uchar green", "property uchar blue"]
  header += [f"element face {faces.shape[0]}", "property list uchar int vertex_indices", "end_header"]
  with open(path, 'wb') as f:
    f.write(("\n".join(header) + "\n").encode('ascii'))
    f.write(vertex_rows.tobytes())
    f.write(face_rows.tobytes())


def fuse_scene(gaussians, cameras: Sequence[CameraParams], config, volume: TSDFVolume, *, alpha_min: float = 0.5,
               batch: int = 8, use_sh: Optional[bool] = None) -> TSDFVolume:
  """Render every camera's depth (``render_gaussians`` + ``render_geometry(normals=False)``, ``.depth`` with
  ``alpha_min``) and fuse it into ``volume``, ``batch`` frames per ``integrate`` call, the rendered image as colour when
  the volume has colour.  Under ``no_grad``.  Bitwise equal to the same loop written by hand, whatever ``batch`` is.
  ``use_sh`` defaults to whether ``gaussians.feature`` holds SH coefficients ``(N, 3, K)``.

  The F = 2 wide pass of ``render_geometry`` dominates the cost per frame, not the fusion: this is an offline
  operation.  Returns ``volume``."""
  from .geometry import render_geometry
  from .renderer import render_gaussians
  if not isinstance(volume, TSDFVolume):
    raise TypeError(f"volume must be a TSDFVolume (got {type(volume).__name__})")
  cameras = [cameras] if isinstance(cameras, CameraParams) else list(cameras)
  if not cameras or not all(isinstance(c, CameraParams) for c in cameras):
    raise TypeError("cameras must be a non-empty sequence of CameraParams")
  if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
    raise ValueError(f"batch must be a positive integer (got {batch!r})")
  if use_sh is None:
    use_sh = gaussians.feature.dim() == 3
  with torch.no_grad():
    for begin in range(0, len(cameras), batch):
      chunk = cameras[begin:begin + batch]
      depths, images = [], []
      for camera in chunk:
        rendering = render_gaussians(gaussians, camera, config, use_sh=use_sh)
        depths.append(render_geometry(rendering, gaussians, normals=False, alpha_min=alpha_min).depth)
        if volume.colour is not None:
          images.append(rendering.image[..., :3])
      volume.integrate(torch.stack(depths), chunk, colour=torch.stack(images) if images else None)
  return volume


__all__ = ["TSDFVolume", "TriangleMesh", "save_mesh_ply", "fuse_scene", "MAX_SAMPLES", "CAMERA_CHUNK"]
