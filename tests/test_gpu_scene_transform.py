"""-m gpu: ``Gaussians3D.transformed`` / ``rotate_sh`` / ``ms_scene_transform`` (csrc/scene_transform.hip).

The reference of every field is a float64 torch restatement written here from the definitions — ``s R p + t``,
``log_scaling + ln s``, the xyzw Hamilton product ``q_R (x) q`` (``rotation_to_quat``: w >= 0) and ``M_l(R) c_l`` per band with
``sh_rotation_matrices`` — evaluated on the very values the kernel reads.

Shapes: with B = MS_SCENE_XFORM_ROWS = 256 rows per workgroup, n in {1, B - 1, B, B + 1, 2 B + 3}: one short block, a
full one, a second block of one row, and a third.  Features: plain (n, 3) colours, degrees 0..3 with f = 3 (degree 3:
whole 16-byte pieces; degree 2 float32: 36-byte vectors, a ragged 4-byte tail; f = 3: three LDS chunks per full block)
and f = 1 at degree 2.  Transform: s = 1.7, a seeded random R, |t| about 10.  ``log_scaling`` is drawn from [-4, -2]:
with ln 1.7 = 0.53 (and ln 0.8 = -0.22 in the composition test) no intermediate is in a higher binade than the final
value, so "2 ulp" (of the final value) is a bound that two correctly rounded additions keep.

float32 bounds (<= 7-term FMA dots with weights of modulus <= 1, matrix entries rounded once to float32): a rotated
coefficient within 2e-6 max|c| of its band row, position within 1e-6 (s |p|_1 + |t|_inf), log_scaling within 2 ulp,
rotation within 1e-6 |q|.  float64: 1e-12 of the (reference) row's largest magnitude.

Composition and round trip in float32 are two applications, each within the bounds above on its own input, the first
one's error carried through the second one's linear part (norm s for the position, 1 for quaternion and bands, with
sqrt(3), 2 and sqrt(2 l + 1) between the row norms used): the bounds are added that way, see ``two_step_bounds``.
"""
import functools
import math

import pytest
import torch

from taichi_splatting_amd import (Gaussians3D, RasterConfig, _lib, frame, load_ply, render_gaussians, rotate_sh,
                                  save_ply, sh_rotation_matrices)
from taichi_splatting_amd.data_types import _quat_to_mat
from taichi_splatting_amd.spherical_harmonics import rotation_to_quat
from taichi_splatting_amd.perspective.params import CameraParams
from taichi_splatting_amd.testing import random_3d_gaussians, random_camera

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64 = torch.float64
B = _lib.SCENE_XFORM_ROWS
SIZES = [1, B - 1, B, B + 1, 2 * B + 3]
KINDS = {'colours': (None, 3), 'deg0': (0, 3), 'deg1': (1, 3), 'deg2': (2, 3), 'deg3': (3, 3), 'deg2_f1': (2, 1)}
DTYPES = {'f32': torch.float32, 'f64': torch.float64}
FIELDS = ('position', 'log_scaling', 'rotation', 'alpha_logit', 'feature')


def random_rotation(seed):
  q = torch.randn(4, generator=torch.Generator().manual_seed(seed), dtype=F64)
  return _quat_to_mat(q / q.norm())


def similarity(s, R, t):
  m = torch.eye(4, dtype=F64)
  m[:3, :3] = s * R
  m[:3, 3] = torch.as_tensor(t, dtype=F64)
  return m


def inverse_similarity(m):
  """exact last row, unlike torch.inverse"""
  s = float(torch.linalg.det(m[:3, :3])) ** (1.0 / 3.0)
  R = m[:3, :3] / s
  return similarity(1.0 / s, R.T, -(R.T @ m[:3, 3]) / s)


M_A = similarity(1.7, random_rotation(1), [6.0, -7.0, 5.0])          # |t| = 10.5
M_B = similarity(0.8, random_rotation(2), [-2.0, 3.0, 1.5])


@functools.lru_cache(maxsize=None)
def scene(n, kind, dtype):
  """A seeded scene on the CPU in ``dtype`` (shared: never modified).  Row 0's quaternion is zero when n > 1."""
  degree, f = KINDS[kind]
  gen = torch.Generator().manual_seed(1000 + n)
  r = lambda *shape: torch.randn(*shape, generator=gen, dtype=F64)
  rotation = r(n, 4) * torch.exp(0.5 * r(n, 1))                        # not normalised
  if n > 1:
    rotation[0] = 0.0
  feature = torch.rand(n, 3, generator=gen, dtype=F64) if degree is None else 0.5 * r(n, f, (degree + 1) ** 2)
  log_scaling = -4.0 + 2.0 * torch.rand(n, 3, generator=gen, dtype=F64)
  return Gaussians3D(position=3.0 * r(n, 3), log_scaling=log_scaling, rotation=rotation, alpha_logit=r(n, 1),
                     feature=feature, batch_size=(n,)).to(dtype=dtype)


def quat_mul(a, q):
  """Hamilton product a (x) q, xyzw: R(a (x) q) = R(a) R(q)"""
  ax, ay, az, aw = a.unbind(-1)
  x, y, z, w = q.unbind(-1)
  return torch.stack([aw * x + ax * w + ay * z - az * y, aw * y - ax * z + ay * w + az * x,
                      aw * z + ax * y - ay * x + az * w, aw * w - ax * x - ay * y - az * z], dim=-1)


def restated(g, m, rotate=True):
  """the transformed scene in float64 from the definitions, on the values of ``g`` (any dtype, CPU)"""
  s = float(torch.linalg.det(m[:3, :3])) ** (1.0 / 3.0)
  R, t = m[:3, :3] / s, m[:3, 3]
  out = dict(position=s * g.position.double() @ R.T + t, log_scaling=g.log_scaling.double() + math.log(s),
             rotation=quat_mul(rotation_to_quat(R), g.rotation.double()), alpha_logit=g.alpha_logit.double(),
             feature=g.feature.double().clone())
  if g.feature.ndim == 3 and rotate:
    degree = math.isqrt(g.feature.shape[2]) - 1
    for l, M in enumerate(sh_rotation_matrices(R, degree)):
      band = slice(l * l, (l + 1) * (l + 1))
      out['feature'][:, :, band] = g.feature.double()[:, :, band] @ M.T
  return out, (s, R, t)


def band_max(feature):
  """(N, F, K): max |c| of each coefficient's band row"""
  out = torch.empty_like(feature)
  for l in range(math.isqrt(feature.shape[2])):
    band = slice(l * l, (l + 1) * (l + 1))
    out[:, :, band] = feature[:, :, band].abs().amax(dim=2, keepdim=True)
  return out


def ulp32(x64):
  x = x64.float().abs()
  return (torch.nextafter(x, torch.full_like(x, float('inf'))) - x).double()


def one_step_bounds(g, srt, ref):
  """per-element float32 bounds of one application on the input ``g`` (module docstring)"""
  s, R, t = srt
  p1 = g.position.double().abs().sum(dim=1, keepdim=True)
  return dict(position=(1e-6 * (s * p1 + t.abs().max())).expand(-1, 3),
              log_scaling=2.0 * ulp32(ref['log_scaling']),
              rotation=(1e-6 * g.rotation.double().norm(dim=1, keepdim=True)).expand(-1, 4),
              feature=2e-6 * band_max(g.feature.double()) if g.feature.ndim == 3 else None)


def row_magnitude_bounds(ref, rel):
  out = {k: (rel * ref[k].abs().amax(dim=1, keepdim=True)).expand_as(ref[k]) for k in ('position', 'log_scaling', 'rotation')}
  out['feature'] = rel * band_max(ref['feature']) if ref['feature'].ndim == 3 else None
  return out


def check(got, ref, bounds, what, rotated=True):
  # q_R and -q_R are the same rotation: two applications may give the rows of one of the product with the other sign
  flip = -1.0 if float((got.rotation.cpu().double() * ref['rotation']).sum()) < 0 else 1.0
  for key in ('position', 'log_scaling', 'rotation'):
    err = ((flip if key == 'rotation' else 1.0) * getattr(got, key).cpu().double() - ref[key]).abs()
    over = err - bounds[key]
    assert bool((over <= 0).all()), f"{what}: {key} off by {float(err.max()):.3e}, {float(over.max()):.3e} beyond its bound"
  if got.feature.ndim == 3 and got.feature.shape[2] > 1 and rotated:
    err = (got.feature.cpu().double() - ref['feature']).abs()
    over = err - bounds['feature']
    assert bool((over <= 0).all()), f"{what}: feature off by {float(err.max()):.3e}, {float(over.max()):.3e} beyond its bound"
    assert torch.equal(got.feature[:, :, 0].cpu().double(), ref['feature'][:, :, 0]), f"{what}: band 0 changed"


def bits(x):
  return x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int64)


def same_bits(a, b):
  return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ---- 1. the kernel against the restatement ----------------------------------------------------------------------------

@pytest.mark.parametrize('kind', list(KINDS))
@pytest.mark.parametrize('dt', list(DTYPES))
def test_transformed_matches_the_float64_restatement(dt, kind):
  dtype = DTYPES[dt]
  for n in SIZES:
    g = scene(n, kind, dtype)
    ref, srt = restated(g, M_A)
    gd = g.to(DEV)
    got = gd.transformed(M_A)
    bounds = one_step_bounds(g, srt, ref) if dtype == torch.float32 else row_magnitude_bounds(ref, 1e-12)
    check(got, ref, bounds, f"{dt} {kind} n={n}")
    assert same_bits(got.alpha_logit, gd.alpha_logit) and got.alpha_logit.data_ptr() == gd.alpha_logit.data_ptr()
    if n > 1:
      assert bool((got.rotation[0] == 0).all()), "a zero quaternion must stay zero"
    if KINDS[kind][0] in (None, 0):
      assert got.feature.data_ptr() == gd.feature.data_ptr(), "colours / degree 0: the feature is shared"
    for key in FIELDS:                                                  # the input scene is untouched
      assert same_bits(getattr(gd, key).cpu(), getattr(g, key)), key
    # rotate_sh=False: the feature is the input's, bit for bit; the geometry is the same as above
    plain = gd.transformed(M_A, rotate_sh=False)
    assert plain.feature.data_ptr() == gd.feature.data_ptr()
    for key in ('position', 'log_scaling', 'rotation'):
      assert same_bits(getattr(plain, key), getattr(got, key)), key
    # rotate_sh alone
    if KINDS[kind][0] is not None:
      alone = rotate_sh(gd.feature, srt[1])
      assert same_bits(alone, got.feature)
      assert (alone.data_ptr() == gd.feature.data_ptr()) == (KINDS[kind][0] == 0)


# ---- 2. in place ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', list(KINDS))
@pytest.mark.parametrize('dt', list(DTYPES))
def test_in_place_equals_out_of_place_bitwise(dt, kind):
  dtype = DTYPES[dt]
  for n in SIZES:
    g = scene(n, kind, dtype).to(DEV)
    want = g.transformed(M_A)
    work = g.clone()
    pointers = [getattr(work, k).data_ptr() for k in FIELDS]
    back = work.transformed(M_A, inplace=True)
    assert back is work and [getattr(work, k).data_ptr() for k in FIELDS] == pointers
    for key in FIELDS:
      assert same_bits(getattr(work, key), getattr(want, key)), (n, key)
    # every tensor a slice [1 : n + 1] of a guarded buffer: the degree-2 float32 feature then starts 108 bytes into its
    # allocation (4-byte aligned only); rows 0 and n + 1 must come back untouched
    guarded = {k: torch.full((n + 2,) + tuple(getattr(g, k).shape[1:]), -77.0, dtype=dtype, device=DEV) for k in FIELDS}
    for k in FIELDS:
      guarded[k][1:n + 1] = getattr(g, k)
    sliced = Gaussians3D(**{k: guarded[k][1:n + 1] for k in FIELDS}, batch_size=(n,))
    copied = sliced.transformed(M_A)                                     # misaligned source, aligned destination
    sliced.transformed(M_A, inplace=True)
    for key in FIELDS:
      assert same_bits(guarded[key][1:n + 1], getattr(want, key)), (n, key, 'sliced, in place')
      assert same_bits(getattr(copied, key), getattr(want, key)), (n, key, 'sliced source')
      assert bool((guarded[key][0] == -77.0).all()) and bool((guarded[key][n + 1] == -77.0).all()), (n, key, 'guard rows')
    if KINDS[kind][0] not in (None, 0):
      R = restated(scene(n, kind, dtype), M_A)[1][1]
      buffer = torch.full((n + 2,) + tuple(g.feature.shape[1:]), -77.0, dtype=dtype, device=DEV)
      buffer[1:n + 1] = g.feature
      assert rotate_sh(buffer[1:n + 1], R, out=buffer[1:n + 1]).data_ptr() == buffer[1:n + 1].data_ptr()
      assert same_bits(buffer[1:n + 1], want.feature)
      assert bool((buffer[0] == -77.0).all()) and bool((buffer[n + 1] == -77.0).all())


# ---- 3. render equivariance -------------------------------------------------------------------------------------------

EQUIVARIANCE_SEED = 5
EQUIVARIANCE_SIZE = (64, 48)


def equivariance_case(seed=EQUIVARIANCE_SEED):
  """(scene, camera, m, moved camera) in float64 on the CPU: 300 gaussians in front of a random camera, degree-3
  features with band >= 1 coefficients ~ N(0, 0.3).  Moved camera: T' = diag(s, s, s, 1) T m^-1 (its 3x3 block is a
  rotation again), near and far times s."""
  torch.manual_seed(seed)
  camera = random_camera(image_size=EQUIVARIANCE_SIZE)
  g = random_3d_gaussians(300, camera, scale_factor=1.0, alpha_range=(0.1, 0.9))
  feature = 0.3 * torch.randn(300, 3, 16)
  feature[:, :, 0] = (torch.rand(300, 3) - 0.5) / 0.28209479177387814
  g = g.replace(feature=feature).to(dtype=F64)
  camera = camera.to(dtype=F64)
  camera.T_camera_world[3] = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=F64)   # (a float32 inverse leaves 1e-8 there)
  s = 1.7
  m = similarity(s, random_rotation(seed + 100), [4.0, -9.0, 2.5])
  moved = CameraParams(projection=camera.projection.clone(),
                       T_camera_world=torch.diag(torch.tensor([s, s, s, 1.0], dtype=F64)) @ camera.T_camera_world @ torch.inverse(m),
                       near_plane=camera.near_plane * s, far_plane=camera.far_plane * s, image_size=camera.image_size)
  return g, camera, m, moved


@pytest.mark.parametrize('tile_size', [16, 8])
def test_moved_scene_renders_the_same_image_from_the_moved_camera(tile_size):
  """Fails without the SH rotation: with ``rotate_sh=False`` (what ``transform_rigid`` does) the image moves by more
  than 1e-2 (oracle/render.py in float64 on the CPU, this seed, both tile sizes: 0.72 without the rotation, 5e-14 with it)."""
  g, camera, m, moved = equivariance_case()
  g, camera, moved = g.to(DEV), camera.to(device=DEV), moved.to(device=DEV)
  config = RasterConfig(tile_size=tile_size, pixel_stride=(2, 2) if tile_size == 16 else (1, 1))
  frame.USE_FRAME = False                                   # the modular float64 path
  try:
    with torch.no_grad():
      want = render_gaussians(g, camera, config, use_sh=True)
      got = render_gaussians(g.transformed(m), moved, config, use_sh=True)
      unrotated = render_gaussians(g.transformed(m, rotate_sh=False), moved, config, use_sh=True)
  finally:
    frame.USE_FRAME = True
  assert want.points.idx.shape[0] > 150 and float(want.image_weight.max()) > 0.5
  assert torch.equal(got.points.idx, want.points.idx)
  assert float((got.image - want.image).abs().max()) <= 1e-9
  assert float((got.image_weight - want.image_weight).abs().max()) <= 1e-9
  assert float(((got.points.depths - 1.7 * want.points.depths) / (1.7 * want.points.depths)).abs().max()) <= 1e-9
  assert float((unrotated.image - want.image).abs().max()) > 1e-2
  assert float((unrotated.image_weight - want.image_weight).abs().max()) <= 1e-9      # only the colours are wrong


# ---- 4. composition and round trips -----------------------------------------------------------------------------------

def two_step_bounds(g, mid, m1, m2):
  """float32: the second application's bounds on its own input ``mid`` plus the first one's carried through the
  second's linear part (module docstring).  ``mid``: the float64 restatement of the first step."""
  ref1, srt1 = restated(g, m1)
  first = one_step_bounds(g, srt1, ref1)
  mid_scene = Gaussians3D(**{k: mid[k] for k in FIELDS}, batch_size=g.batch_size)
  ref2, srt2 = restated(mid_scene, m2)
  second = one_step_bounds(mid_scene, srt2, ref2)
  out = dict(position=second['position'] + math.sqrt(3.0) * srt2[0] * first['position'].amax(dim=1, keepdim=True),
             log_scaling=None,
             rotation=second['rotation'] + 2.0 * first['rotation'])
  if first['feature'] is not None:
    width = torch.empty(g.feature.shape[2], dtype=F64)
    for l in range(math.isqrt(g.feature.shape[2])):
      width[l * l:(l + 1) * (l + 1)] = math.sqrt(2 * l + 1)
    out['feature'] = second['feature'] + width * first['feature']
  else:
    out['feature'] = None
  return out


@pytest.mark.parametrize('dt', list(DTYPES))
def test_composition_and_round_trip(dt):
  dtype = DTYPES[dt]
  n = 2 * B + 3
  for m1, m2 in ((M_A, M_B), (M_A, inverse_similarity(M_A))):
    g = scene(n, 'deg3', dtype)
    ref, _ = restated(g, m2 @ m1)
    got = g.to(DEV).transformed(m1).transformed(m2)
    if dtype == torch.float64:
      bounds = row_magnitude_bounds(ref, 1e-11)
    else:
      bounds = two_step_bounds(g, restated(g, m1)[0], m1, m2)
      bounds['log_scaling'] = 2.0 * ulp32(ref['log_scaling'])
      once = g.to(DEV).transformed(m2 @ m1)
      check(once, ref, one_step_bounds(g, restated(g, m2 @ m1)[1], ref), f"{dt} one application of the product")
    check(got, ref, bounds, f"{dt} two applications")


def test_transformed_scene_survives_a_ply_round_trip(tmp_path):
  g = scene(B + 1, 'deg3', torch.float32).to(DEV).transformed(M_A)
  save_ply(g, tmp_path / 'moved.ply')
  back = load_ply(tmp_path / 'moved.ply', device='cuda')
  for key in FIELDS:
    assert same_bits(getattr(back, key), getattr(g, key)), key


# ---- 5. graph capture -------------------------------------------------------------------------------------------------

def test_rotate_sh_captures_into_a_graph():
  """One kernel node, no host read, allocation or synchronisation inside the call: captured in place, replayed twice
  on fresh copies of the input."""
  R = random_rotation(9)
  feature = scene(2 * B + 3, 'deg3', torch.float32).feature.to(DEV)
  eager = rotate_sh(feature, R)
  static = feature.clone()
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    rotate_sh(static, R, out=static)
  for _ in range(2):
    static.copy_(feature)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(static, eager)


# ---- the tool ----------------------------------------------------------------------------------------------------------

def test_render_scene_tool_moves_the_scene(tmp_path):
  """``tools/render_scene.py --transform "y 90"``: the tool's cameras orbit the scene's median in the x-z plane, and a
  quarter turn about y maps that orbit onto itself one view on (N is odd and int(0.05 N) + int(0.95 N) = N - 1, so the
  median and the 5-95 % extent the orbit is built from turn with the scene exactly): view v - 1 of the moved scene is view
  v of the original.  float32 through the frame path: two renders whose inputs differ in the last bits agree to 1e-4
  except where a (pixel, splat) pair sits at the blend gate, which moves a pixel by at most alpha_threshold x |colour|
  = 4e-3 per pair — asserted: mean below 1e-4, every pixel below 1e-2.  Without the SH rotation the views differ by 0.1
  and more (degree-3 coefficients ~ N(0, 0.3))."""
  import json
  import subprocess
  import sys
  from pathlib import Path
  import numpy as np
  n = 257
  assert int(0.05 * n) + int(0.95 * n) == n - 1
  torch.manual_seed(3)
  camera = random_camera(image_size=(64, 48))
  g = random_3d_gaussians(n, camera, scale_factor=1.0, alpha_range=(0.1, 0.9))
  g = g.replace(feature=torch.cat([(torch.rand(n, 3, 1) - 0.5) / 0.28209479177387814, 0.3 * torch.randn(n, 3, 15)], dim=2))
  save_ply(g, tmp_path / 'scene.ply')
  tool = str(Path(__file__).resolve().parent.parent / 'tools' / 'render_scene.py')
  images = {}
  for name, extra in (('original', []), ('moved', ['--transform', 'y 90'])):
    done = subprocess.run([sys.executable, tool, str(tmp_path / 'scene.ply'), '--views', '4', '--size', '64', '48',
                           '--out', str(tmp_path / name)] + extra, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr[-2000:]
    report = json.loads(done.stdout.strip().splitlines()[-1])
    assert report['transform'] == (extra[1] if extra else None) and report['n'] == n
    images[name] = [np.load(tmp_path / name / f'view_{v:03d}.npy').astype(np.float64) for v in range(4)]
  assert max(float(np.abs(i).max()) for i in images['original']) > 0.2
  for v in range(4):
    diff = np.abs(images['moved'][(v - 1) % 4] - images['original'][v])
    assert float(diff.mean()) < 1e-4 and float(diff.max()) < 1e-2, (v, float(diff.mean()), float(diff.max()))


# ---- 6. errors --------------------------------------------------------------------------------------------------------

def test_errors():
  g = scene(B + 1, 'deg3', torch.float32)
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    g.transformed(M_A)
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    rotate_sh(g.feature, M_A[:3, :3] / 1.7)
  leaf = g.to(DEV).requires_grad_(True)
  before = leaf.feature.detach().clone()
  with pytest.raises(RuntimeError, match="require grad"):
    leaf.transformed(M_A, inplace=True)
  assert same_bits(leaf.feature.detach(), before)
  with torch.no_grad():
    assert leaf.transformed(M_A, inplace=True) is leaf
  assert same_bits(leaf.position.detach(), g.to(DEV).transformed(M_A).position)
  with pytest.raises(ValueError, match="cannot represent"):
    g.to(DEV).transformed(torch.diag(torch.tensor([1.0, 1.0, -1.0, 1.0])))
  with pytest.raises(TypeError):
    g.to(DEV).to(dtype=torch.float16).transformed(M_A)
