"""Host-side tests of the geometry feature (no GPU): argument validation of gaussian_normals, render_geometry and
normal_consistency_loss and of their C-ABI entry points (the checks come before any launch), and the yardstick itself —
tests/geometry_oracle.py must be right before the kernels are held to it."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from taichi_splatting_amd import (CameraParams, Gaussians3D, GeometryImages, gaussian_normals, normal_consistency,
                                  normal_consistency_loss, render_geometry, _lib)
from tests import geometry_oracle as go


def gaussians(n=4, dtype=torch.float32):
  return Gaussians3D(position=torch.zeros((n, 3), dtype=dtype), log_scaling=torch.zeros((n, 3), dtype=dtype),
                     rotation=torch.ones((n, 4), dtype=dtype), alpha_logit=torch.zeros((n, 1), dtype=dtype),
                     feature=torch.zeros((n, 3), dtype=dtype), batch_size=(n,))


def camera(w=8, h=6):
  return CameraParams(projection=torch.tensor([10., 10., 4., 3.]), T_camera_world=torch.eye(4), near_plane=0.1,
                      far_plane=100., image_size=(w, h))


def test_gaussian_normals_arguments():
  g = gaussians()
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    gaussian_normals(g, torch.zeros(3))
  with pytest.raises(ValueError, match="3-element"):
    gaussian_normals(g, torch.zeros(4))
  with pytest.raises(TypeError, match="dtype or device"):
    gaussian_normals(g, torch.zeros(3, dtype=torch.float64))
  with pytest.raises(TypeError, match="float32 or float64"):
    gaussian_normals(gaussians(dtype=torch.float16), torch.zeros(3, dtype=torch.float16))
  bad = SimpleNamespace(position=torch.zeros((4, 3)), log_scaling=torch.zeros((5, 3)), rotation=torch.ones((4, 4)))
  with pytest.raises(ValueError, match="log_scaling"):
    gaussian_normals(bad, torch.zeros(3))


def test_normal_consistency_arguments():
  accum, proj = torch.ones((6, 8, 5)), torch.tensor([10., 10., 4., 3.])
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    normal_consistency(accum, 0, 1, 2, proj)
  with pytest.raises(ValueError, match="distinct channels"):
    normal_consistency(accum, 0, 2, 2, proj)                      # alpha inside the normal channels
  with pytest.raises(ValueError, match="distinct channels"):
    normal_consistency(accum, 0, 1, 3, proj)                      # the normal runs off the image
  with pytest.raises(ValueError, match="distinct channels"):
    normal_consistency(torch.ones((6, 8, 4)), 0, 1, 2, proj[:4])
  with pytest.raises(ValueError, match=r"\(H, W, F\)"):
    normal_consistency(accum[0], 0, 1, 2, proj)
  with pytest.raises(ValueError, match="alpha_min > 0"):
    normal_consistency(accum, 0, 1, 2, proj, alpha_min=0.0)
  with pytest.raises(ValueError, match="projection"):
    normal_consistency(accum, 0, 1, 2, proj[:3])
  with pytest.raises(NotImplementedError, match="detach it"):
    normal_consistency(accum, 0, 1, 2, proj.clone().requires_grad_(True))
  with pytest.raises(ValueError, match="pixel_weight"):
    normal_consistency(accum, 0, 1, 2, proj, pixel_weight=torch.ones((8, 6)))
  with pytest.raises(TypeError, match="dtype or device"):
    normal_consistency(accum, 0, 1, 2, proj.double())
  # the GeometryImages form: without normal channels there is nothing to compare
  no_normals = GeometryImages(accum=torch.ones((6, 8, 2)), camera=camera())
  with pytest.raises(ValueError, match="normals=True"):
    normal_consistency_loss(no_normals)
  with pytest.raises(ValueError, match="normals=True"):
    no_normals.normal_sum
  with pytest.raises(ValueError, match="depth_variance=True"):
    no_normals.depth_sq_sum
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    normal_consistency_loss(GeometryImages(accum=accum, camera=camera(), normal_offset=2))


def test_geometry_image_properties():
  """the torch properties on a hand-made accumulation: depth and variance under alpha_min are 0, the normal is unit or 0"""
  accum = torch.zeros((2, 2, 6), dtype=torch.float64)
  accum[0, 0] = torch.tensor([1.6, 0.8, 3.4, 0.0, 0.0, -0.4], dtype=torch.float64)       # z = 2, z^2 mean 4.25
  accum[0, 1] = torch.tensor([0.3, 0.2, 0.5, 0.0, 0.0, 0.0], dtype=torch.float64)        # under alpha_min; a zero normal
  geo = GeometryImages(accum=accum, camera=camera(), depth_sq_offset=2, normal_offset=3)
  assert geo.depth[0, 0] == 2.0 and geo.depth[0, 1] == 0.0 and geo.depth[1, 1] == 0.0
  assert abs(float(geo.depth_variance[0, 0]) - 0.25) < 1e-15 and geo.depth_variance[0, 1] == 0.0
  assert torch.equal(geo.normal[0, 0], torch.tensor([0., 0., -1.], dtype=torch.float64))
  assert torch.equal(geo.normal[0, 1], torch.zeros(3, dtype=torch.float64))
  assert abs(float(geo.distortion[0, 0]) - (0.8 * 3.4 - 1.6 ** 2)) < 1e-15
  assert torch.isfinite(geo.depth).all() and torch.isfinite(geo.normal).all()


def test_render_geometry_needs_a_frame_rendering():
  """a rendering that does not come from the frame executor raises what render_features raises"""
  from taichi_splatting_amd import Rendering, RasterConfig
  rendering = Rendering(image=torch.zeros((6, 8, 3)), image_weight=torch.zeros((6, 8)), points=None, camera=camera(),
                        config=RasterConfig())
  with pytest.raises(ValueError, match="alpha_min"):
    render_geometry(rendering, gaussians(), alpha_min=0.0)
  with pytest.raises(ValueError, match="frame executor"):
    render_geometry(rendering, gaussians(), normals=False)
  with pytest.raises(RuntimeError, match="no CPU fallback"):          # the normals come first, and they need the GPU
    render_geometry(rendering, gaussians())


def test_c_abi_argument_checks(lib):
  need = ctypes.c_size_t(0)
  fwd, bwd = lib.ms_normal_consistency_fwd, lib.ms_normal_consistency_bwd
  assert fwd(None, None, None, 100, 200, 5, 0, 1, 2, _lib.MS_F32, 0.5, None, ctypes.byref(need), None, None, None) == 0
  assert need.value >= 8 * 4 * 7                                    # one double per 64 x 16 tile
  assert fwd(None, None, None, 100, 200, 5, 0, 1, 3, _lib.MS_F32, 0.5, None, ctypes.byref(need), None, None, None) == -1
  assert b'offsets' in lib.ms_last_error_string()
  assert fwd(None, None, None, 100, 200, 5, 2, 1, 2, _lib.MS_F32, 0.5, None, ctypes.byref(need), None, None, None) == -1
  assert b'overlap' in lib.ms_last_error_string()
  assert fwd(None, None, None, 100, 200, 4, 0, 1, 2, _lib.MS_F32, 0.5, None, ctypes.byref(need), None, None, None) == -1
  assert fwd(None, None, None, 100, 200, 5, 0, 1, 2, _lib.MS_F32, 0.0, None, ctypes.byref(need), None, None, None) == -1
  assert b'alpha_min' in lib.ms_last_error_string()
  assert fwd(None, None, None, 0, 200, 5, 0, 1, 2, _lib.MS_F32, 0.5, None, ctypes.byref(need), None, None, None) == -1
  assert fwd(None, None, None, 100, 200, 5, 0, 1, 2, 7, 0.5, None, ctypes.byref(need), None, None, None) == -2
  assert fwd(None, None, None, 100, 200, 5, 0, 1, 2, _lib.MS_F32, 0.5, None, None, None, None, None) == -1
  small = ctypes.c_size_t(8)
  assert fwd(None, None, None, 100, 200, 5, 0, 1, 2, _lib.MS_F32, 0.5, 1, ctypes.byref(small), None, None, None) == -3
  assert fwd(None, None, None, 100, 200, 5, 0, 1, 2, _lib.MS_F32, 0.5, 1, ctypes.byref(need), None, None, None) == -1
  assert b'null pointer' in lib.ms_last_error_string()
  assert bwd(None, None, None, None, 100, 200, 5, 0, 1, 2, _lib.MS_F32, 0.5, None, None) == -1
  assert bwd(1, None, 1, 1, 100, 200, 5, 0, 1, 2, _lib.MS_F64, -1.0, 1, None) == -1
  assert lib.ms_gaussian_normals_fwd(None, None, None, None, 10, _lib.MS_F32, None, None, None) == -1
  assert lib.ms_gaussian_normals_fwd(None, None, None, None, -1, _lib.MS_F32, None, None, None) == -1
  assert lib.ms_gaussian_normals_fwd(None, None, None, None, 10, 5, None, None, None) == -2
  assert lib.ms_gaussian_normals_fwd(None, None, None, None, 0, _lib.MS_F32, None, None, None) == 0      # nothing to do
  assert lib.ms_gaussian_normals_bwd(None, None, None, 10, _lib.MS_F64, None, None) == -1


# ---- the yardstick ----------------------------------------------------------------------------------------------------

def test_oracle_normals_pass_gradcheck_and_follow_the_rules():
  pos, ls, rot, cam, _ = go.make_gaussians(8)
  rot = rot.clone().requires_grad_(True)
  assert torch.autograd.gradcheck(lambda q: go.normals(pos, ls, q, cam), (rot,), eps=1e-6, atol=1e-7)
  n = go.normals(pos, ls, rot, cam).detach()
  assert torch.allclose(n.norm(dim=1), torch.ones(8, dtype=torch.float64), atol=1e-14)
  assert bool(((n * (pos - cam)).sum(1) <= 0).all())                 # every normal faces the camera
  # ties take the lowest index; scaling or negating a quaternion changes nothing
  ident = torch.tensor([[0., 0., 0., 1.]], dtype=torch.float64)
  far = torch.tensor([[0., 0., 5.]], dtype=torch.float64)
  origin = torch.zeros(3, dtype=torch.float64)
  for scales, axis in (([-1., -2., -2.], 1), ([-2., -2., -2.], 0), ([-2., -1., -2.], 0), ([-1., -1., -3.], 2)):
    got = go.normals(far, torch.tensor([scales], dtype=torch.float64), ident, origin)[0]
    want = torch.zeros(3, dtype=torch.float64)
    want[axis] = -1.0 if axis == 2 else 1.0                          # z faces away and is flipped; x, y have n . p = 0: kept
    assert torch.equal(got, want), (scales, got)
  assert torch.allclose(go.normals(pos, ls, -3.0 * rot.detach(), cam), n, atol=1e-14)
  # autograd reaches the rotation alone
  p, s, c = pos.clone().requires_grad_(True), ls.clone().requires_grad_(True), cam.clone().requires_grad_(True)
  go.normals(p, s, rot, c).sum().backward()
  assert p.grad is None and s.grad is None and c.grad is None and rot.grad is not None


def test_oracle_consistency_passes_gradcheck():
  accum, proj, weight = go.make_image(5, 6, 6, (5, 3, 0))
  accum[..., 3] = accum[..., 3].clamp_min(0.7)                       # every stencil counts; nothing at a threshold
  accum[..., 5] = 4.0 * accum[..., 3] * (1 + 0.05 * torch.rand((5, 6), dtype=torch.float64))
  zero = accum[..., 0:3].abs().sum(-1) == 0                         # "0 and no gradient" is a jump no difference follows
  assert int(zero.sum()) == 2
  accum[..., 0:3] = torch.where(zero[..., None], torch.tensor([0.2, 0.1, -0.5], dtype=torch.float64), accum[..., 0:3])
  # with the weight given: the default weight is alpha held constant, which a finite difference cannot hold constant
  x = accum.clone().requires_grad_(True)
  assert torch.autograd.gradcheck(lambda t: go.consistency(t, 5, 3, 0, proj, weight)[0], (x,), eps=1e-6, atol=1e-7)
  loss, nd, grad = go.reference(accum, (5, 3, 0), proj)
  assert float(loss) > 0
  assert bool((grad[..., 4] == 0).all())                             # a channel the loss does not read
  # the default weight is alpha as a constant: its gradient is that of the same weights passed in
  _, _, grad_w = go.reference(accum, (5, 3, 0), proj, accum[..., 3].clone())
  assert torch.equal(grad, grad_w)


def test_oracle_depth_normal_of_a_tilted_plane_is_the_plane_normal():
  proj = go.default_projection(9, 11)
  for normal in ([0.0, 0.0, -1.0], [0.3, -0.2, -1.0], [-0.5, 0.4, -0.8]):
    n = torch.tensor(normal, dtype=torch.float64)
    n = n / n.norm()
    accum = go.plane_image(9, 11, n, -3.0, proj)
    loss, nd, _ = go.reference(accum, (0, 1, 2), proj)
    assert torch.allclose(nd[1:-1, 1:-1], n.expand(7, 9, 3), atol=1e-12), normal
    assert bool((nd[0] == 0).all() and (nd[:, 0] == 0).all() and (nd[-1] == 0).all() and (nd[:, -1] == 0).all())
    assert abs(float(loss)) < 1e-12                                  # normal_sum is the plane's normal too


def test_oracle_degenerate_images_and_cases():
  for shape in ((1, 1), (2, 5), (3, 2)):
    accum, proj, _ = go.make_image(*shape)
    loss, nd, grad = go.reference(accum, (0, 1, 2), proj)
    assert float(loss) == 0.0 and bool((grad == 0).all()) and bool((nd == 0).all())
  accum, proj, _ = go.make_image(3, 3)
  assert float(go.reference(accum, (0, 1, 2), proj)[0]) > 0           # the one interior pixel counts
  # the cases keep away from alpha_min and hold exact zeros
  accum, proj, _ = go.make_image(37, 53)
  alpha = accum[..., 1]
  assert bool(((alpha <= 0.3) | (alpha >= 0.7)).all()) and int((alpha == 0).sum()) >= 6
  assert int((accum[..., 2:5].abs().sum(-1) == 0).sum()) >= 2
