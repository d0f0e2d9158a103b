"""No GPU: the host side of ``Gaussians3D.transformed`` — the SH band rotations ``sh_rotation_matrices`` against
``oracle.sh.rsh_cart`` in float64, the validation of the 4x4 matrix, and the argument checks of ``ms_scene_transform``
(they come before any launch)."""
import ctypes
import functools
import math

import pytest
import torch

from oracle import sh as osh
from taichi_splatting_amd import _lib, sh_rotation_matrices
from taichi_splatting_amd.data_types import similarity_from_matrix, _quat_to_mat
from taichi_splatting_amd.spherical_harmonics import rotation_to_quat

F64 = torch.float64
P = torch.tensor([[0., -1., 0.], [0., 0., 1.], [-1., 0., 0.]], dtype=F64)     # band 1 is k (-y, z, -x) = k P d
BANDS = [slice(l * l, (l + 1) * (l + 1)) for l in range(4)]


@functools.lru_cache(maxsize=None)
def rotations():
  """five seeded random rotations (uniform unit quaternions), shared: never modified"""
  gen = torch.Generator().manual_seed(2024)
  q = torch.randn(5, 4, generator=gen, dtype=F64)
  return tuple(_quat_to_mat(q / q.norm(dim=1, keepdim=True)))


@functools.lru_cache(maxsize=None)
def directions():
  d = torch.randn(1000, 3, generator=torch.Generator().manual_seed(7), dtype=F64)
  return d / d.norm(dim=1, keepdim=True)


def eye(l):
  return torch.eye(2 * l + 1, dtype=F64)


@pytest.mark.parametrize('i', range(5))
def test_defining_identity_and_orthogonality(i):
  R = rotations()[i]
  M = sh_rotation_matrices(R, 3)
  assert [tuple(m.shape) for m in M] == [(1, 1), (3, 3), (5, 5), (7, 7)]
  assert all(m.dtype == F64 and m.device.type == 'cpu' for m in M)
  y, y_rot = osh.rsh_cart(directions(), 3), osh.rsh_cart(directions() @ R.T, 3)
  for l, band in enumerate(BANDS):
    assert (y_rot[:, band] - y[:, band] @ M[l].T).abs().max().item() <= 1e-12, l      # Y_l(R d) = M_l Y_l(d)
    assert (M[l] @ M[l].T - eye(l)).abs().max().item() <= 1e-12, l
  assert torch.equal(M[0], torch.ones(1, 1, dtype=F64))
  assert (M[1] - P @ R @ P.T).abs().max().item() <= 1e-14


@pytest.mark.parametrize('i', range(5))
def test_homomorphism(i):
  R1, R2 = rotations()[i], rotations()[(i + 1) % 5]
  M1, M2, M12 = sh_rotation_matrices(R1, 3), sh_rotation_matrices(R2, 3), sh_rotation_matrices(R1 @ R2, 3)
  for l in range(4):
    assert (M12[l] - M1[l] @ M2[l]).abs().max().item() <= 1e-12, l


def test_identity_and_lower_degrees():
  for l, m in enumerate(sh_rotation_matrices(torch.eye(3, dtype=F64), 3)):
    assert (m - eye(l)).abs().max().item() <= 1e-15, l
  R = rotations()[0]
  full = sh_rotation_matrices(R, 3)
  for degree in range(3):
    part = sh_rotation_matrices(R.float(), degree)       # a float32 rotation is accepted (validated at 1e-5)
    assert len(part) == degree + 1
    for a, b in zip(part, full):
      assert (a - b).abs().max().item() <= 1e-6


@pytest.mark.parametrize('i', range(5))
def test_rotated_coefficients_keep_the_colours(i):
  """sum c' . Y(R d) = sum c . Y(d); with c left alone the colours move by O(1), so this check can fail."""
  R = rotations()[i]
  M = sh_rotation_matrices(R, 3)
  c = torch.randn(16, generator=torch.Generator().manual_seed(100 + i), dtype=F64)
  c_rot = torch.cat([M[l] @ c[band] for l, band in enumerate(BANDS)])
  colour = osh.rsh_cart(directions(), 3) @ c
  y_rot = osh.rsh_cart(directions() @ R.T, 3)
  assert (y_rot @ c_rot - colour).abs().max().item() <= 1e-12
  assert (y_rot @ c - colour).abs().max().item() > 0.1


def test_quarter_turn_about_z():
  """(x, y, z) -> (-y, x, z): band 1 = k (-y, z, -x) becomes k (-x, z, y), i.e. (c1, c2, c3) -> (c3, c2, -c1); four
  quarter turns are the identity on every band."""
  Rz = torch.tensor([[0., -1., 0.], [1., 0., 0.], [0., 0., 1.]], dtype=F64)
  M = sh_rotation_matrices(Rz, 3)
  c = torch.tensor([0.3, -1.1, 0.7], dtype=F64)
  assert (M[1] @ c - torch.tensor([0.7, -1.1, -0.3], dtype=F64)).abs().max().item() <= 1e-14
  assert (M[1] - P @ Rz @ P.T).abs().max().item() <= 1e-14
  for l in range(4):
    assert (torch.linalg.matrix_power(M[l], 4) - eye(l)).abs().max().item() <= 1e-12, l
    assert (M[l] - eye(l)).abs().max().item() > 0.5 or l == 0


def test_rotation_quaternion_is_accurate_in_every_branch():
  """unit, w >= 0, and R(q_R) = R to 1e-15, also where one component is tiny (half turns about each axis, nearly)"""
  half_turns = []
  for axis in range(3):
    for eps in (0.0, 1e-9, -1e-9):
      q = torch.full((4,), eps, dtype=F64)
      q[axis] = 1.0
      half_turns.append(_quat_to_mat(q / q.norm()))
  for R in list(rotations()) + half_turns + [torch.eye(3, dtype=F64)]:
    q = rotation_to_quat(R)
    assert q.dtype == F64 and abs(float(q.norm()) - 1.0) <= 1e-15 and float(q[3]) >= 0.0
    assert (_quat_to_mat(q) - R).abs().max().item() <= 2e-15


def similarity(s, R, t):
  m = torch.eye(4, dtype=F64)
  m[:3, :3] = s * R
  m[:3, 3] = torch.as_tensor(t, dtype=F64)
  return m


def test_similarity_is_recovered():
  R = rotations()[1]
  s, r, t = similarity_from_matrix(similarity(1.7, R, [1., -2., 3.]))
  assert abs(s - 1.7) <= 1e-14 and (r - R).abs().max().item() <= 1e-14 and t.tolist() == [1., -2., 3.]
  s, r, t = similarity_from_matrix(similarity(0.25, R, [0., 0., 0.]).float())
  assert abs(s - 0.25) <= 1e-6 and (r - R).abs().max().item() <= 1e-6


def test_invalid_transforms_raise():
  R = rotations()[2]
  shear = torch.eye(4, dtype=F64)
  shear[0, 1] = 0.2
  last_row = similarity(1.0, R, [0., 0., 0.])
  last_row[3, 0] = 1e-3
  cases = {
    'reflection': torch.diag(torch.tensor([1., 1., -1., 1.], dtype=F64)),
    'shear': shear,
    'non-uniform scale': torch.diag(torch.tensor([1., 2., 1., 1.], dtype=F64)),
    'last row': last_row,
    'singular': torch.diag(torch.tensor([1., 1., 0., 1.], dtype=F64)),
  }
  for name, m in cases.items():
    with pytest.raises(ValueError):
      similarity_from_matrix(m)
  for name in ('reflection', 'shear', 'non-uniform scale'):
    with pytest.raises(ValueError, match="quaternion and an isotropic log_scaling offset cannot represent"):
      similarity_from_matrix(cases[name])
  for bad in (torch.eye(3, dtype=F64), torch.zeros(3, 4, dtype=F64), torch.zeros(16, dtype=F64), [[1.0]]):
    with pytest.raises(ValueError):
      similarity_from_matrix(bad)
  # the rotation itself
  for bad in (torch.diag(torch.tensor([1., 1., -1.], dtype=F64)), shear[:3, :3], 2.0 * R, torch.eye(4, dtype=F64),
              torch.zeros(3, dtype=F64)):
    with pytest.raises(ValueError):
      sh_rotation_matrices(bad, 3)
  for degree in (4, -1, 1.0, True):
    with pytest.raises(ValueError):
      sh_rotation_matrices(R, degree)


def test_transformed_validates_before_touching_the_scene():
  from taichi_splatting_amd import Gaussians3D
  g = Gaussians3D(position=torch.zeros(2, 3), log_scaling=torch.zeros(2, 3), rotation=torch.ones(2, 4),
                  alpha_logit=torch.zeros(2, 1), feature=torch.zeros(2, 3, 16), batch_size=(2,))
  with pytest.raises(ValueError, match="cannot represent"):
    g.transformed(torch.diag(torch.tensor([1., 1., -1., 1.])))
  with pytest.raises(ValueError):
    g.transformed(torch.eye(3))
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    g.transformed(torch.eye(4))


def test_render_scene_tool_refuses_a_reflection_before_reading_the_file(tmp_path):
  import subprocess
  import sys
  tool = _lib.PACKAGE_DIR.parent / 'tools' / 'render_scene.py'
  for text, message in (('1 0 0 0  0 1 0 0  0 0 -1 0  0 0 0 1', 'cannot represent'), ('w 90', 'AXIS DEG')):
    done = subprocess.run([sys.executable, str(tool), str(tmp_path / 'absent.ply'), '--transform', text],
                          capture_output=True, text=True, timeout=120)
    assert done.returncode != 0 and message in done.stderr, done.stderr[-500:]


def call(lib, *, pairs=(1, 1, 1, 1, 1, 1, 1, 1), n=10, f=3, sh_degree=3, dtype=_lib.MS_F32, transform=True):
  """ms_scene_transform with dummy non-null pointers (word-aligned: 8): a rejected call launches nothing"""
  values = (ctypes.c_double * _lib.SCENE_XFORM_VALUES)() if transform else None
  return lib.ms_scene_transform(*[8 if p else None for p in pairs], n, f, sh_degree, dtype, values, None)


def test_scene_transform_argument_errors(lib):
  assert call(lib, sh_degree=4) == -1
  assert b'sh_degree' in lib.ms_last_error_string()
  assert call(lib, sh_degree=0) == -1 and b'sh_degree' in lib.ms_last_error_string()
  assert call(lib, pairs=(1, 1, 1, 1, 1, 1, 0, 0), sh_degree=4, n=0) == 0       # no feature: the degree is not read
  for k, name in enumerate((b'position', b'log_scaling', b'rotation', b'feature')):
    for side in (0, 1):
      pairs = [1] * 8
      pairs[2 * k + side] = 0
      assert call(lib, pairs=tuple(pairs)) == -1, (name, side)
      assert name in lib.ms_last_error_string()
  assert call(lib, n=-1) == -1 and b'n >= 0' in lib.ms_last_error_string()
  assert call(lib, f=0) == -1 and b'f' in lib.ms_last_error_string()
  assert call(lib, dtype=7) == -1 and b'dtype' in lib.ms_last_error_string()
  assert call(lib, transform=False) == -1 and b'transform' in lib.ms_last_error_string()
  assert call(lib, n=0) == 0
  assert call(lib, n=0, dtype=_lib.MS_F64) == 0
  assert call(lib, pairs=(0,) * 8) == 0                                         # nothing to do
  assert lib.ms_scene_transform(4, 4, None, None, None, None, None, None, 10, 3, 3, _lib.MS_F64,
                                (ctypes.c_double * 100)(), None) == -1          # a double array at a 4-byte address
  assert b'aligned' in lib.ms_last_error_string()
  assert _lib.SCENE_XFORM_ROWS == 256 and _lib.SCENE_XFORM_VALUES == 100
  header = (_lib.PACKAGE_DIR.parent / 'include' / 'mi355_splat.h').read_text()
  assert '#define MS_SCENE_XFORM_ROWS 256' in header and 'MS_SCENE_XFORM_VALUES = 100' in header
