"""scene_io on the host: load_ply / save_ply / read_ply_header against PLY bytes that THIS FILE builds with struct.pack,
property by property, so that the reader and the writer are each held against an independent statement of the format and
never only against each other.

The golden scene has 3 gaussians of SH degree 1 in the 3DGS property order.  Value of vertex i, property j (position in
that order): 100 (i + 1) + j, a distinct small integer, exact in float32: a swapped column is a wrong number, not a
tolerance.  (The normals are zero in the golden file because save_ply writes zeros and test_golden_save compares bytes; the
reordered and ascii variants carry non-zero normals, which must be ignored.)
"""
import os
import struct

import numpy as np
import pytest
import torch

import taichi_splatting_amd as tsa
from taichi_splatting_amd import Gaussians3D, scene_io
from taichi_splatting_amd.data_types import SH_C0
from taichi_splatting_amd.scene_io import load_ply, read_ply_header, save_ply

ORDER_DEG1 = (['x', 'y', 'z', 'nx', 'ny', 'nz', 'f_dc_0', 'f_dc_1', 'f_dc_2'] + [f'f_rest_{i}' for i in range(9)] +
              ['opacity', 'scale_0', 'scale_1', 'scale_2', 'rot_0', 'rot_1', 'rot_2', 'rot_3'])
N_GOLD = 3
PACK = {'float': '<f', 'float32': '<f', 'double': '<d', 'float64': '<d', 'uchar': '<B', 'int': '<i'}


def value(i, name):
  return float(100 * (i + 1) + ORDER_DEG1.index(name))


def golden_rows(normals=False):
  rows = [{name: value(i, name) for name in ORDER_DEG1} for i in range(N_GOLD)]
  if not normals:
    for row in rows:
      row.update(nx=0.0, ny=0.0, nz=0.0)
  return rows


def ply_bytes(props, rows, fmt='binary_little_endian', header_extra=(), trailing_header=(), trailing_body=b'', count=None):
  """props: [(name, ply type)]; rows: [{name: value}].  Header and body written out by hand."""
  lines = ['ply', f'format {fmt} 1.0', *header_extra, f'element vertex {len(rows) if count is None else count}']
  lines += [f'property {kind} {name}' for name, kind in props]
  lines += [*trailing_header, 'end_header']
  out = ('\n'.join(lines) + '\n').encode('ascii')
  for row in rows:
    if fmt == 'ascii':
      out += (' '.join(repr(row[name]) if kind in ('float', 'double') else str(int(row[name])) for name, kind in props) + '\n').encode()
    else:
      for name, kind in props:
        out += struct.pack(PACK[kind], int(row[name]) if kind in ('uchar', 'int') else row[name])
  return out + trailing_body


def write(tmp_path, name, data):
  path = tmp_path / name
  path.write_bytes(data)
  return path


def golden_file(tmp_path):
  return write(tmp_path, 'golden.ply', ply_bytes([(name, 'float') for name in ORDER_DEG1], golden_rows()))


def expected_golden():
  """The mapping of the issue, written out: xyzw from wxyz, channel-major f_rest."""
  v = lambda names: torch.tensor([[value(i, name) for name in names] for i in range(N_GOLD)], dtype=torch.float32)
  feature = torch.empty((N_GOLD, 3, 4))
  for i in range(N_GOLD):
    for c in range(3):
      feature[i, c, 0] = value(i, f'f_dc_{c}')
      for k in range(3):
        feature[i, c, 1 + k] = value(i, f'f_rest_{c * 3 + k}')
  return Gaussians3D(position=v(['x', 'y', 'z']), log_scaling=v(['scale_0', 'scale_1', 'scale_2']),
                     rotation=v(['rot_1', 'rot_2', 'rot_3', 'rot_0']), alpha_logit=v(['opacity']), feature=feature,
                     batch_size=(N_GOLD,))


def assert_same(a, b):
  for key in ('position', 'log_scaling', 'rotation', 'alpha_logit', 'feature'):
    x, y = getattr(a, key), getattr(b, key)
    assert x.dtype == y.dtype == torch.float32 and x.shape == y.shape, f"{key}: {x.shape} {x.dtype} / {y.shape} {y.dtype}"
    assert torch.equal(x.cpu().view(torch.int32), y.cpu().view(torch.int32)), f"{key} differs"
  assert tuple(a.batch_size) == tuple(b.batch_size)


# ---- 1-4: reading ------------------------------------------------------------------------------------------------------

def test_golden_load(tmp_path):
  g = load_ply(golden_file(tmp_path))
  assert isinstance(g, Gaussians3D) and g.position.device.type == 'cpu'
  assert g.alpha_logit.shape == (N_GOLD, 1) and g.feature.shape == (N_GOLD, 3, 4)
  assert_same(g, expected_golden())
  rot_0 = torch.tensor([value(i, 'rot_0') for i in range(N_GOLD)])
  assert torch.equal(g.rotation[:, 3], rot_0)                                              # w is LAST here, FIRST in the file
  assert torch.equal(g.feature[:, 1, 2], torch.tensor([value(i, f'f_rest_{1 * 3 + 1}') for i in range(N_GOLD)]))
  assert_same(Gaussians3D.load_ply(golden_file(tmp_path)), g)


def test_header(tmp_path):
  path = golden_file(tmp_path)
  h = read_ply_header(path)
  assert h.format == 'binary_little_endian' and h.count == N_GOLD
  assert h.properties == tuple((name, 'f4') for name in ORDER_DEG1)
  data = path.read_bytes()
  assert data[:h.offset].endswith(b'end_header\n') and len(data) - h.offset == N_GOLD * len(ORDER_DEG1) * 4


def test_reordered_properties_unknown_columns_comments_and_a_trailing_element(tmp_path):
  props = [(name, 'float') for name in reversed(ORDER_DEG1)]
  props.insert(3, ('confidence', 'float'))
  props.insert(11, ('label', 'uchar'))
  props.insert(20, ('time', 'float'))
  rows = golden_rows(normals=True)
  for i, row in enumerate(rows):
    row.update(confidence=-7.0 - i, label=200 + i, time=9999.0)
  data = ply_bytes(props, rows, header_extra=['comment made by hand', 'obj_info nothing to see', 'comment'],
                   trailing_header=['element face 0', 'property list uchar int vertex_indices'])
  path = write(tmp_path, 'reordered.ply', data)
  assert_same(load_ply(path), expected_golden())
  h = read_ply_header(path)
  assert [name for name, _ in h.properties] == [name for name, _ in props] and dict(h.properties)['label'] == 'u1'


def test_ascii(tmp_path):
  data = ply_bytes([(name, 'float') for name in ORDER_DEG1], golden_rows(normals=True), fmt='ascii',
                   header_extra=['comment ascii'], trailing_header=['element face 1', 'property list uchar int vertex_indices'],
                   trailing_body=b'3 0 1 2\n')
  path = write(tmp_path, 'ascii.ply', data)
  assert_same(load_ply(path), expected_golden())
  assert_same(load_ply(path, chunk_rows=2), expected_golden())


@pytest.mark.parametrize('fmt', ('binary_little_endian', 'ascii'))
def test_double_positions_equal_the_float32_cast(tmp_path, fmt):
  props = [(name, 'double' if name in 'xyz' else 'float') for name in ORDER_DEG1]
  rows = golden_rows()
  for i, row in enumerate(rows):
    row.update(x=0.1 + i, y=1.0 / 3.0 - i, z=1e-3 * (i + 1) + 2.0 ** -40)                  # none representable in float32
  path = write(tmp_path, 'double.ply', ply_bytes(props, rows, fmt=fmt))
  g = load_ply(path, chunk_rows=2)
  want = torch.from_numpy(np.array([[row['x'], row['y'], row['z']] for row in rows], dtype=np.float64).astype(np.float32))
  assert g.position.dtype == torch.float32 and torch.equal(g.position, want)
  assert_same(g.replace(position=expected_golden().position), expected_golden())


# ---- 5-6: writing ------------------------------------------------------------------------------------------------------

def test_golden_save(tmp_path):
  golden = golden_file(tmp_path).read_bytes()
  out = tmp_path / 'saved.ply'
  save_ply(expected_golden(), out)
  assert out.read_bytes() == golden
  expected_golden().save_ply(out, chunk_rows=1)
  assert out.read_bytes() == golden
  assert golden.startswith(b'ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\n')
  assert sorted(os.listdir(tmp_path)) == ['golden.ply', 'saved.ply']                        # no temporary file left


def random_scene(n, form, seed=0):
  gen = torch.Generator().manual_seed(seed)
  feature = torch.rand((n, 3), generator=gen) if form == 'rgb' else torch.randn((n, 3, (form + 1) ** 2), generator=gen)
  return Gaussians3D(position=torch.randn((n, 3), generator=gen), log_scaling=torch.randn((n, 3), generator=gen),
                     rotation=torch.randn((n, 4), generator=gen) * 3.0,                     # NOT unit length: must survive
                     alpha_logit=torch.randn((n, 1), generator=gen), feature=feature, batch_size=(n,))


@pytest.mark.parametrize('n', (5, 0))
@pytest.mark.parametrize('form', (0, 1, 2, 3, 'rgb'))
def test_round_trip(tmp_path, form, n):
  g = random_scene(n, form)
  path = tmp_path / 'scene.ply'
  save_ply(g, path, chunk_rows=2)                      # slab boundary inside the scene, last slab partial
  h = read_ply_header(path)
  degree = 0 if form == 'rgb' else form
  assert h.count == n and len(h.properties) == 17 + 3 * ((degree + 1) ** 2 - 1)
  assert os.path.getsize(path) == h.offset + n * 4 * len(h.properties)
  back = load_ply(path, chunk_rows=2)
  assert tuple(back.batch_size) == (n,)
  if form == 'rgb':
    assert back.feature.shape == (n, 3, 1)
    colours = 0.5 + SH_C0 * back.feature[:, :, 0]
    assert torch.allclose(colours, g.feature, rtol=0.0, atol=1e-6)
    assert torch.equal(load_ply(path, sh_degree=None).feature, colours)
    assert_same(back.replace(feature=g.feature), g)
  else:
    assert_same(back, g)
    assert_same(load_ply(path), back)                  # one slab


def test_other_feature_widths_are_refused(tmp_path):
  g = random_scene(4, 1)
  for feature in (torch.zeros((4, 4)), torch.zeros((4, 3, 5)), torch.zeros((4, 1, 4)), torch.zeros((4, 3, 25))):
    with pytest.raises(ValueError, match='feature'):
      save_ply(g.replace(feature=feature), tmp_path / 'no.ply')
  assert os.listdir(tmp_path) == []


# ---- 7: sh_degree ------------------------------------------------------------------------------------------------------

def test_sh_degree_argument(tmp_path):
  g3, g1 = random_scene(5, 3, seed=1), random_scene(5, 1, seed=2)
  p3, p1 = tmp_path / 'deg3.ply', tmp_path / 'deg1.ply'
  save_ply(g3, p3)
  save_ply(g1, p1)
  assert_same(load_ply(p3, sh_degree=1, chunk_rows=2), g3.replace(feature=g3.feature[:, :, :4].contiguous()))
  assert_same(load_ply(p3, sh_degree=0), g3.replace(feature=g3.feature[:, :, :1].contiguous()))
  assert_same(load_ply(p3, sh_degree=3), g3)
  up = load_ply(p1, sh_degree=3, chunk_rows=2)
  assert up.feature.shape == (5, 3, 16) and torch.equal(up.feature[:, :, :4], g1.feature)
  assert torch.count_nonzero(up.feature[:, :, 4:]) == 0
  rgb = load_ply(p3, sh_degree=None)
  assert rgb.feature.shape == (5, 3) and torch.equal(rgb.feature, 0.5 + SH_C0 * g3.feature[:, :, 0])
  for bad in (4, -1, 'three', 1.0, True):
    with pytest.raises(ValueError, match='sh_degree'):
      load_ply(p3, sh_degree=bad)


# ---- 8: the SH convention ----------------------------------------------------------------------------------------------

def sh_colour_3dgs(sh, d):
  """Colour of SH coefficients sh (16,) seen along the unit direction d = point - camera in the 3DGS convention: the
  real spherical harmonics with the constants and signs published with the method, + 0.5, float64."""
  C0 = 0.28209479177387814
  C1 = 0.4886025119029199
  C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
  C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
        1.445305721320277, -0.5900435899266435)
  x, y, z = d
  xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
  c = C0 * sh[0]
  c = c - C1 * y * sh[1] + C1 * z * sh[2] - C1 * x * sh[3]
  c = (c + C2[0] * xy * sh[4] + C2[1] * yz * sh[5] + C2[2] * (2.0 * zz - xx - yy) * sh[6] + C2[3] * xz * sh[7] +
       C2[4] * (xx - yy) * sh[8])
  c = (c + C3[0] * y * (3.0 * xx - yy) * sh[9] + C3[1] * xy * z * sh[10] + C3[2] * y * (4.0 * zz - xx - yy) * sh[11] +
       C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy) * sh[12] + C3[4] * x * (4.0 * zz - xx - yy) * sh[13] +
       C3[5] * z * (xx - yy) * sh[14] + C3[6] * x * (xx - 3.0 * yy) * sh[15])
  return c + 0.5


def test_sh_basis_is_the_3dgs_convention():
  from oracle import sh as osh
  gen = torch.Generator().manual_seed(5)
  axes = torch.tensor([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=torch.float64)
  free = torch.randn((10, 3), generator=gen, dtype=torch.float64)
  dirs = torch.cat([axes, free / free.norm(dim=1, keepdim=True)])                          # 16 fixed unit directions
  # |coefficient| <= 0.05: the colour stays inside (0, 1), where neither convention's clamp acts
  params = (torch.rand((16, 3, 16), generator=gen, dtype=torch.float64) - 0.5) * 0.1
  camera = torch.zeros(3, dtype=torch.float64)
  ours = osh.evaluate_sh_at(params, dirs, torch.arange(16), camera)                        # direction = point - camera
  assert float(ours.min()) > 0.0 and float(ours.max()) < 1.0
  worst = 0.0
  for v in range(16):
    for c in range(3):
      want = sh_colour_3dgs([float(s) for s in params[v, c]], [float(s) for s in dirs[v]])
      worst = max(worst, abs(float(ours[v, c]) - want))
  print(f"oracle.sh against the 3DGS formula, degree 3, 16 directions: largest difference {worst:.2e}")
  assert worst <= 1e-6
  # and band by band: one coefficient at a time, so that two swapped or sign-flipped basis functions cannot cancel
  for k in range(16):
    one = torch.zeros((16, 3, 16), dtype=torch.float64)
    one[:, :, k] = 0.2
    got = osh.evaluate_sh_at(one, dirs, torch.arange(16), camera)
    for v in range(16):
      sh = [0.2 if j == k else 0.0 for j in range(16)]
      assert abs(float(got[v, 0]) - sh_colour_3dgs(sh, [float(s) for s in dirs[v]])) <= 1e-6, f"basis function {k}"


# ---- 9: errors ---------------------------------------------------------------------------------------------------------

def float_props(names=ORDER_DEG1):
  return [(name, 'float') for name in names]


def bad_big_endian():
  return ply_bytes(float_props(), golden_rows(), fmt='binary_big_endian'), 'binary_big_endian'


def bad_missing_property():
  return ply_bytes(float_props([n for n in ORDER_DEG1 if n != 'scale_1']), golden_rows()), 'missing required property scale_1'


def bad_missing_f_rest_index():
  names = [n if n != 'f_rest_4' else 'f_rest_11' for n in ORDER_DEG1]
  rows = [dict(row, f_rest_11=1.0) for row in golden_rows()]
  return ply_bytes(float_props(names), rows), 'missing required property f_rest_4'


def bad_f_rest_count():
  return ply_bytes(float_props([n for n in ORDER_DEG1 if n != 'f_rest_8']), golden_rows()), '8 f_rest'


def bad_integer_property():
  return ply_bytes([(n, 'int' if n == 'opacity' else 'float') for n in ORDER_DEG1], golden_rows()), 'opacity has integer type'


def bad_list_property():
  header = ['ply', 'format binary_little_endian 1.0', 'element vertex 0']
  header += [f'property list uchar float {n}' if n == 'rot_2' else f'property float {n}' for n in ORDER_DEG1]
  return ('\n'.join(header + ['end_header']) + '\n').encode(), 'rot_2 has list type'


def bad_short_binary_body():
  return ply_bytes(float_props(), golden_rows())[:-1], 'shorter than count x row size'


def bad_short_ascii_body():
  return ply_bytes(float_props(), golden_rows()[:2], fmt='ascii', count=3), 'shorter than count x row size'


def bad_no_end_header():
  data = ply_bytes(float_props(), golden_rows(), header_extra=['comment ' + 'x' * 1000] * 70)
  assert data.index(b'end_header') > 64 * 1024
  return data, 'no end_header'


def bad_truncated_header():
  return b'ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\n', 'no end_header'


BAD = [bad_big_endian, bad_missing_property, bad_missing_f_rest_index, bad_f_rest_count, bad_integer_property,
       bad_list_property, bad_short_binary_body, bad_short_ascii_body, bad_no_end_header, bad_truncated_header]


@pytest.mark.parametrize('case', BAD, ids=[f.__name__ for f in BAD])
def test_errors_name_the_file_and_the_cause(tmp_path, case):
  data, cause = case()
  path = write(tmp_path, case.__name__ + '.ply', data)
  with pytest.raises(ValueError) as info:
    load_ply(path)
  assert str(path) in str(info.value) and cause in str(info.value), str(info.value)


def test_a_failed_save_leaves_no_file(tmp_path):
  path = tmp_path / 'no_such_directory' / 'scene.ply'
  with pytest.raises(OSError):
    save_ply(random_scene(5, 1), path)
  assert not path.exists() and not path.parent.exists() and os.listdir(tmp_path) == []
  # a save that fails halfway keeps what was under the name before and removes its temporary file
  kept = tmp_path / 'kept.ply'
  save_ply(random_scene(5, 1), kept)
  before = kept.read_bytes()
  broken = random_scene(5, 1, seed=9)
  broken = broken.replace(rotation=broken.rotation)
  object.__setattr__(broken, 'log_scaling', torch.zeros((5, 2)))      # the first slab's gather raises after the header is out
  with pytest.raises(RuntimeError):
    save_ply(broken, kept)
  assert kept.read_bytes() == before and os.listdir(tmp_path) == ['kept.ply']


def test_public_surface():
  assert tsa.load_ply is load_ply and tsa.save_ply is save_ply and tsa.read_ply_header is read_ply_header
  assert {'load_ply', 'save_ply', 'read_ply_header'} <= set(tsa.__all__)
  assert scene_io.property_names(3)[:9] == ('x', 'y', 'z', 'nx', 'ny', 'nz', 'f_dc_0', 'f_dc_1', 'f_dc_2')
  assert len(scene_io.property_names(3)) == 62 and scene_io.property_names(0)[-8:] == (
    'opacity', 'scale_0', 'scale_1', 'scale_2', 'rot_0', 'rot_1', 'rot_2', 'rot_3')
