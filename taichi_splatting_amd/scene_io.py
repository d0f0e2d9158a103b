"""Scenes in and out: ``Gaussians3D`` <-> the binary PLY of the original 3D Gaussian Splatting trainer (no reference
counterpart; every splatting viewer and trainer reads this file).

Field mapping (file -> ``Gaussians3D``), columns looked up by NAME, never by position:

  x y z            -> position (N, 3)
  scale_0..2       -> log_scaling (N, 3)      the file already holds logs
  opacity          -> alpha_logit (N, 1)      the file already holds the logit
  rot_0..3         -> rotation (N, 4)         the file is WXYZ, ``Gaussians3D.rotation`` is XYZW: rotation[:, 3] = rot_0,
                                              rotation[:, 0:3] = rot_1..3.  Permuted, NOT normalised (the kernels
                                              normalise; a round trip is bit-exact)
  f_dc_c           -> feature[:, c, 0]        c = 0..2 (red, green, blue)
  f_rest_{c*M + k} -> feature[:, c, 1 + k]    CHANNEL-MAJOR, M = (D + 1)^2 - 1, k = 0..M-1.  D follows from the number of
                                              f_rest_* properties (3 M for a D in 0..3; none at all: degree 0)
  nx ny nz, others -> ignored on load; ``save_ply`` writes nx ny nz as zeros so that the layout is the one other tools expect

SH basis: the real basis and the + 0.5 offset of ``csrc/sh.hip`` / ``oracle/sh.py`` ARE the 3DGS convention — same
constants, same signs (-C1 y, +C1 z, -C1 x, ...), same order through degree 3, direction = point - camera — so
coefficients are copied, not converted (``tests/test_scene_io_host.py::test_sh_basis_is_the_3dgs_convention``).

A ``Gaussians3D`` whose ``feature`` is (N, 3) colours is saved as degree 0 with f_dc = (rgb - 0.5) / SH_C0; loading returns
the SH form (N, 3, 1), and the colours are ``0.5 + SH_C0 * feature[:, :, 0]`` (``load_ply(sh_degree=None)`` returns that).

Read: ``binary_little_endian 1.0`` and ``ascii 1.0``; properties in any order; ``float`` / ``float32`` and ``double`` /
``float64`` (converted to float32); ``comment`` and ``obj_info`` lines; elements after ``vertex`` are ignored.
Written: ``binary_little_endian`` only, float32, the 3DGS property order
``x y z nx ny nz f_dc_0..2 f_rest_* opacity scale_0..2 rot_0..3``.

Data path.  THERE IS NO KERNEL HERE, on purpose: the header is parsed on the host; the body is read through ``np.memmap``
in slabs of ``chunk_rows`` rows, each an (rows, P) float32 table with one column per property; a slab goes to the device
through ONE reused pinned staging buffer; there the five tensors are filled with one ``index_select`` each over column
lists built once from the header.  Rows that mix float32 with other types are unpacked through a structured dtype on the
host for that slab.  ``save_ply`` is the inverse: one (rows, <= 62) table gathered on the device, one device-to-host copy
per slab, ``tofile``.  A degree-3 scene of 6 M gaussians is 1.49 GB: reading it costs seconds, the device-side unpack moves
the same bytes once at memory bandwidth (``profiles/scene_io.txt``), and slabbing keeps the extra host memory at one slab.
"""
from __future__ import annotations

import os
import re
import time
from typing import NamedTuple, Optional, Tuple, Union

import numpy as np
import torch

from .data_types import SH_C0, Gaussians3D

__all__ = ['PlyHeader', 'read_ply_header', 'load_ply', 'save_ply', 'load_points_ply']

HEADER_LIMIT = 64 * 1024          # `end_header` must lie in the first 64 KiB

# PLY scalar type names -> numpy type codes (byte order added where the file is read)
_SCALARS = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2',
            'uint16': 'u2', 'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4',
            'double': 'f8', 'float64': 'f8'}
_LIST = 'list'

_POSITION = ('x', 'y', 'z')
_NORMALS = ('nx', 'ny', 'nz')
_RGB = ('red', 'green', 'blue')
_DC = ('f_dc_0', 'f_dc_1', 'f_dc_2')
_OPACITY = ('opacity',)
_SCALE = ('scale_0', 'scale_1', 'scale_2')
_ROT_WXYZ = ('rot_0', 'rot_1', 'rot_2', 'rot_3')
_ROT_XYZW = ('rot_1', 'rot_2', 'rot_3', 'rot_0')
_REST_COUNTS = {0: 0, 9: 1, 24: 2, 45: 3}          # number of f_rest_* properties -> SH degree


class PlyHeader(NamedTuple):
  format: str                                   # 'binary_little_endian' | 'ascii' | 'binary_big_endian'
  count: int                                    # vertices
  properties: Tuple[Tuple[str, str], ...]       # ordered (name, numpy type code such as 'f4', or 'list') of the vertex element
  offset: int                                   # first byte of the body


def read_ply_header(path) -> PlyHeader:
  """Parse the header of a PLY file: format, vertex count, the vertex element's (name, dtype) properties in file order
  and the offset of the body.  Raises ``ValueError`` naming the file for anything that is not a PLY header."""
  path = os.fspath(path)
  with open(path, 'rb') as f:
    head = f.read(HEADER_LIMIT)
  if not head.startswith(b'ply'):
    raise ValueError(f"{path}: not a PLY file (it does not begin with 'ply')")
  end = re.search(rb'(?:^|\n)end_header\r?\n', head)
  if end is None:
    raise ValueError(f"{path}: no end_header line in the first {HEADER_LIMIT // 1024} KiB")
  fmt, count, properties, element = None, None, [], None
  for line in head[:end.start()].decode('ascii', errors='replace').splitlines()[1:]:
    words = line.split()
    if not words or words[0] in ('comment', 'obj_info'):
      continue
    if words[0] == 'format' and len(words) == 3:
      fmt = words[1]
      if words[2] != '1.0':
        raise ValueError(f"{path}: PLY version {words[2]} is not 1.0")
    elif words[0] == 'element' and len(words) == 3:
      element = words[1]
      if element == 'vertex':
        count = int(words[2])
      elif count is None and int(words[2]) != 0:
        raise ValueError(f"{path}: element {element} ({words[2]} entries) comes before element vertex")
    elif words[0] == 'property' and element is not None:
      if element != 'vertex':
        continue
      if words[1] == 'list' and len(words) == 5:
        properties.append((words[4], _LIST))
      elif len(words) == 3 and words[1] in _SCALARS:
        properties.append((words[2], _SCALARS[words[1]]))
      else:
        raise ValueError(f"{path}: cannot parse header line {line!r}")
    else:
      raise ValueError(f"{path}: cannot parse header line {line!r}")
  if fmt not in ('binary_little_endian', 'binary_big_endian', 'ascii'):
    raise ValueError(f"{path}: missing or unknown format line (format {fmt})")
  if count is None or count < 0:
    raise ValueError(f"{path}: the header has no element vertex")
  return PlyHeader(fmt, count, tuple(properties), end.end())


def _columns(path: str, header: PlyHeader):
  """(degree of the file, {property name: column}) after checking that every property a scene needs is there as a float."""
  column = {}
  for i, (name, _) in enumerate(header.properties):
    column.setdefault(name, i)
  rest = [name for name, _ in header.properties if re.fullmatch(r'f_rest_\d+', name)]
  if len(set(rest)) not in _REST_COUNTS:
    raise ValueError(f"{path}: {len(set(rest))} f_rest_* properties match no SH degree (0, 9, 24 or 45 for degree 0..3)")
  degree = _REST_COUNTS[len(set(rest))]
  required = _POSITION + _DC + tuple(f'f_rest_{i}' for i in range(len(set(rest)))) + _OPACITY + _SCALE + _ROT_WXYZ
  for name in required:
    if name not in column:
      raise ValueError(f"{path}: missing required property {name}")
    kind = header.properties[column[name]][1]
    if kind == _LIST:
      raise ValueError(f"{path}: required property {name} has list type, expected float or double")
    if kind[0] != 'f':
      raise ValueError(f"{path}: required property {name} has integer type ({kind}), expected float or double")
  for name, kind in header.properties:
    if kind == _LIST:
      raise ValueError(f"{path}: list property {name} in element vertex (rows of variable length are not supported)")
  return degree, column


def _host_slabs(path: str, header: PlyHeader, wanted, chunk_rows: int):
  """Yield (first row, last row + 1, (rows, P) float32 table) over the body.  For a file whose properties are all float32
  the table is a view of the memory map: nothing is read before the consumer copies it."""
  n, p = header.count, len(header.properties)
  if header.format == 'ascii':
    with open(path, 'rb') as f:
      f.seek(header.offset)
      for r0 in range(0, n, chunk_rows):
        r1 = min(n, r0 + chunk_rows)
        lines = [f.readline() for _ in range(r1 - r0)]
        try:
          table = np.array(b' '.join(lines).split(), dtype=np.float64)
        except ValueError as e:
          raise ValueError(f"{path}: rows {r0}..{r1 - 1} of the ascii body: {e}") from None
        if table.size != (r1 - r0) * p:
          raise ValueError(f"{path}: body is shorter than count x row size: rows {r0}..{r1 - 1} hold {table.size} values, "
                           f"expected {r1 - r0} rows x {p} properties")
        yield r0, r1, table.reshape(r1 - r0, p).astype(np.float32)
    return

  row = np.dtype({'names': [f'c{i}' for i in range(p)], 'formats': ['<' + kind for _, kind in header.properties]})
  body = os.path.getsize(path) - header.offset
  if body < n * row.itemsize:
    raise ValueError(f"{path}: body is shorter than count x row size: {body} bytes after the header, "
                     f"{n} x {row.itemsize} = {n * row.itemsize} expected")
  if all(kind == 'f4' for _, kind in header.properties):
    table = np.memmap(path, dtype='<f4', mode='r', offset=header.offset, shape=(n, p))
    for r0 in range(0, n, chunk_rows):
      r1 = min(n, r0 + chunk_rows)
      yield r0, r1, table[r0:r1]
    return
  rows = np.memmap(path, dtype=row, mode='r', offset=header.offset, shape=(n,))
  for r0 in range(0, n, chunk_rows):
    r1 = min(n, r0 + chunk_rows)
    slab = rows[r0:r1]
    table = np.zeros((r1 - r0, p), dtype=np.float32)        # columns nobody asked for stay zero
    for c in wanted:
      table[:, c] = slab[f'c{c}']
    yield r0, r1, table


def _load(path, device, sh_degree, chunk_rows: int, timings: Optional[dict] = None) -> Gaussians3D:
  """``load_ply``; ``timings`` (tools/bench_scene_io.py, tools/render_scene.py) receives ``read_s`` (host: file -> staging
  buffer), ``upload_ms`` and ``unpack_ms`` (device events, summed over the slabs)."""
  path = os.fspath(path)
  device = torch.device(device)
  if not (sh_degree == 'file' or sh_degree is None or
          (isinstance(sh_degree, int) and not isinstance(sh_degree, bool) and 0 <= sh_degree <= 3)):
    raise ValueError(f"sh_degree must be 'file', None or an integer in 0..3, got {sh_degree!r}")
  if not isinstance(chunk_rows, int) or chunk_rows < 1:
    raise ValueError(f"chunk_rows must be a positive integer, got {chunk_rows!r}")
  header = read_ply_header(path)
  if header.format == 'binary_big_endian':
    raise ValueError(f"{path}: binary_big_endian files are not supported (binary_little_endian and ascii are)")
  file_degree, column = _columns(path, header)

  # how many SH coefficients per channel are taken from the file, and how many the result has
  if sh_degree is None:
    taken = kept = 1
  else:
    kept = (file_degree + 1) ** 2 if sh_degree == 'file' else (sh_degree + 1) ** 2
    taken = min(kept, (file_degree + 1) ** 2)
  m = (file_degree + 1) ** 2 - 1
  feature_names = [_DC[c] if k == 0 else f'f_rest_{c * m + k - 1}' for c in range(3) for k in range(taken)]
  fields = [('position', _POSITION), ('log_scaling', _SCALE), ('rotation', _ROT_XYZW), ('alpha_logit', _OPACITY),
            ('feature', feature_names)]
  wanted = sorted({column[name] for _, names in fields for name in names})
  n, p = header.count, len(header.properties)
  out = {key: torch.empty((n, len(names)), dtype=torch.float32, device=device) for key, names in fields}
  select = {key: torch.tensor([column[name] for name in names], dtype=torch.int64, device=device) for key, names in fields}

  on_gpu = device.type == 'cuda'
  timed = timings is not None
  read_s, spans = 0.0, []
  if on_gpu and n > 0:
    stage = torch.empty((min(chunk_rows, n), p), dtype=torch.float32, pin_memory=True)      # the ONE staging buffer
    stage_np = stage.numpy()
    uploaded = torch.cuda.Event()
    stream = torch.cuda.current_stream(device)
  for r0, r1, table in _host_slabs(path, header, wanted, chunk_rows) if n > 0 else ():
    rows = r1 - r0
    if on_gpu:
      if r0 > 0:
        uploaded.synchronize()                    # the previous slab has left the staging buffer
      t0 = time.perf_counter()
      np.copyto(stage_np[:rows], table)           # for a float32 file this is the read: memory map -> pinned buffer
      read_s += time.perf_counter() - t0
      if timed:
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        marks[0].record(stream)
      slab = stage[:rows].to(device, non_blocking=True)
      uploaded.record(stream)
      if timed:
        marks[1].record(stream)
    else:
      t0 = time.perf_counter()
      slab = torch.from_numpy(np.array(table, dtype=np.float32, order='C'))
      read_s += time.perf_counter() - t0
    for key, _ in fields:
      torch.index_select(slab, 1, select[key], out=out[key][r0:r1])
    if on_gpu and timed:
      marks[2].record(stream)
      spans.append(marks)
  if on_gpu and n > 0:
    uploaded.synchronize()
  if timed:
    if spans:
      torch.cuda.synchronize(device)
    timings['read_s'] = read_s
    timings['upload_ms'] = sum(a.elapsed_time(b) for a, b, _ in spans)
    timings['unpack_ms'] = sum(b.elapsed_time(c) for _, b, c in spans)

  feature = out['feature']
  if sh_degree is None:
    feature = 0.5 + SH_C0 * feature
  else:
    feature = feature.view(n, 3, taken)
    if kept > taken:
      feature = torch.cat([feature, feature.new_zeros((n, 3, kept - taken))], dim=2)
  return Gaussians3D(position=out['position'], log_scaling=out['log_scaling'], rotation=out['rotation'],
                     alpha_logit=out['alpha_logit'], feature=feature, batch_size=(n,))


def load_ply(path, *, device='cpu', sh_degree: Union[str, int, None] = 'file', chunk_rows: int = 1 << 20) -> Gaussians3D:
  """Load a 3DGS PLY scene (module docstring: field mapping, formats) onto ``device``.

  ``sh_degree='file'`` keeps the file's degree: feature (N, 3, (D + 1)^2).  An integer 0..3 drops the higher bands or
  pads them with zeros.  ``None`` returns (N, 3) colours from the DC term alone, ``0.5 + SH_C0 * f_dc``.
  ``chunk_rows``: rows per slab (host memory and the pinned staging buffer are one slab).
  Raises ``ValueError`` naming the file and the cause: big-endian, a missing required property, an f_rest count that
  matches no degree, a required property of integer or list type, a body shorter than count x row size, no
  ``end_header`` in the first 64 KiB."""
  return _load(path, device, sh_degree, chunk_rows)


def load_points_ply(path, device='cpu', chunk_rows: int = 1 << 20) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
  """A point cloud — the form ground-truth scans come in — as (points (N, 3) float32, colours (N, 3) float32 in 0..1 or
  None) on ``device``.  Reads ``x y z`` (float or double) and, when all three are there as ``uchar``, ``red green blue``
  (divided by 255); every other property and every element after ``vertex`` (the faces of a mesh file) is ignored.
  ``binary_little_endian`` and ``ascii``; the header and the body go through ``read_ply_header`` and the slab reader of
  ``load_ply``.  ``ValueError`` naming the file for big-endian, a missing or non-float ``x y z``, a list property in the
  vertex element and a short body."""
  path = os.fspath(path)
  header = read_ply_header(path)
  if header.format == 'binary_big_endian':
    raise ValueError(f"{path}: binary_big_endian PLY files are not supported")
  column = {}
  for i, (name, _) in enumerate(header.properties):
    column.setdefault(name, i)
  for name, kind in header.properties:
    if kind == _LIST:
      raise ValueError(f"{path}: list property {name} in element vertex (rows of variable length are not supported)")
  for name in _POSITION:
    if name not in column:
      raise ValueError(f"{path}: missing required property {name}")
    if header.properties[column[name]][1][0] != 'f':
      raise ValueError(f"{path}: required property {name} has integer type ({header.properties[column[name]][1]}), "
                       "expected float or double")
  has_colour = all(name in column and header.properties[column[name]][1] == 'u1' for name in _RGB)
  wanted = [column[name] for name in _POSITION + (_RGB if has_colour else ())]
  table = np.empty((header.count, len(wanted)), dtype=np.float32)
  for r0, r1, slab in _host_slabs(path, header, wanted, chunk_rows):
    table[r0:r1] = slab[:, wanted]
  points = torch.from_numpy(np.ascontiguousarray(table[:, 0:3])).to(device)
  colours = torch.from_numpy(np.ascontiguousarray(table[:, 3:6])).to(device) / 255.0 if has_colour else None
  return points, colours


def property_names(degree: int):
  """The 3DGS property order of a file of SH degree ``degree``."""
  m = (degree + 1) ** 2 - 1
  return _POSITION + _NORMALS + _DC + tuple(f'f_rest_{i}' for i in range(3 * m)) + _OPACITY + _SCALE + _ROT_WXYZ


def _save(gaussians: Gaussians3D, path, chunk_rows: int, timings: Optional[dict] = None) -> None:
  path = os.fspath(path)
  if not isinstance(chunk_rows, int) or chunk_rows < 1:
    raise ValueError(f"chunk_rows must be a positive integer, got {chunk_rows!r}")
  feature = gaussians.feature.detach()
  n = gaussians.position.shape[0]
  if feature.ndim == 2 and feature.shape[1] == 3:
    feature = ((feature.to(torch.float32) - 0.5) / SH_C0).unsqueeze(2)
  elif not (feature.ndim == 3 and feature.shape[1] == 3 and feature.shape[2] in (1, 4, 9, 16)):
    raise ValueError(f"save_ply: feature must be (N, 3) colours or (N, 3, (D + 1)^2) spherical harmonics with D in 0..3, "
                     f"got {tuple(feature.shape)}")
  m = feature.shape[2] - 1
  names = property_names({0: 0, 3: 1, 8: 2, 15: 3}[m])
  p = len(names)
  header = ''.join(['ply\nformat binary_little_endian 1.0\n', f'element vertex {n}\n',
                    *(f'property float {name}\n' for name in names), 'end_header\n']).encode('ascii')
  sources = [t.detach() for t in (gaussians.position, gaussians.alpha_logit, gaussians.log_scaling, gaussians.rotation)]
  position, alpha_logit, log_scaling, rotation = sources
  on_gpu = position.is_cuda
  gather_s = write_s = 0.0

  tmp = f'{path}.tmp{os.getpid()}'         # same directory: os.replace is atomic, a half file never carries the real name
  try:
    with open(tmp, 'wb') as f:
      f.write(header)
      for r0 in range(0, n, chunk_rows):
        r1 = min(n, r0 + chunk_rows)
        t0 = time.perf_counter()
        table = torch.zeros((r1 - r0, p), dtype=torch.float32, device=position.device)     # nx ny nz stay zero
        table[:, 0:3] = position[r0:r1]
        table[:, 6:9] = feature[r0:r1, :, 0]
        table[:, 9:9 + 3 * m] = feature[r0:r1, :, 1:].reshape(r1 - r0, 3 * m)             # channel-major
        table[:, 9 + 3 * m] = alpha_logit[r0:r1, 0]
        table[:, 10 + 3 * m:13 + 3 * m] = log_scaling[r0:r1]
        table[:, 13 + 3 * m] = rotation[r0:r1, 3]                                          # xyzw -> wxyz
        table[:, 14 + 3 * m:17 + 3 * m] = rotation[r0:r1, 0:3]
        host = table.cpu() if on_gpu else table                                            # one copy per slab
        t1 = time.perf_counter()
        host.numpy().tofile(f)
        gather_s, write_s = gather_s + t1 - t0, write_s + time.perf_counter() - t1
    os.replace(tmp, path)
  except BaseException:
    if os.path.exists(tmp):
      os.remove(tmp)
    raise
  if timings is not None:
    timings['gather_copy_s'], timings['write_s'] = gather_s, write_s


def save_ply(gaussians: Gaussians3D, path, *, chunk_rows: int = 1 << 20) -> None:
  """Write ``gaussians`` (on any device) as a ``binary_little_endian`` float32 PLY in the 3DGS property order, normals
  zero.  ``feature`` (N, 3, (D + 1)^2) is written as degree D, (N, 3) colours as degree 0 with f_dc = (rgb - 0.5) / SH_C0;
  any other feature width raises ``ValueError``.  The file is written under a temporary name in the same directory and
  renamed, so an interrupted save leaves nothing under ``path``."""
  _save(gaussians, path, chunk_rows)
