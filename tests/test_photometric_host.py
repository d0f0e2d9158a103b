"""No GPU: the float64 oracle of the photometric loss (tests/photometric_oracle.py) is right, the float32 tolerance the
GPU tests use rejects every mutation of the algorithm, and the C-ABI of csrc/loss.hip answers its argument checks."""
import ctypes
import re

import pytest
import torch

from taichi_splatting_amd import _lib
from tests import photometric_oracle as po


@pytest.mark.parametrize('padding', ['same', 'valid'])
@pytest.mark.parametrize('shape', [(13, 17, 1), (15, 12, 3)])
def test_oracle_equals_the_literal_restatement(shape, padding):
  x, y = po.make_pair('random', *shape)
  a, b = po.ssim_map(x, y, padding), po.literal_ssim_map(x, y, padding)
  assert a.shape == b.shape == ((shape[0], shape[1], shape[2]) if padding == 'same' else (shape[0] - 10, shape[1] - 10, shape[2]))
  assert float((a - b).abs().max()) < 1e-12


@pytest.mark.parametrize('padding', ['same', 'valid'])
def test_oracle_loss_passes_gradcheck(padding):
  x, y = po.make_pair('random', 12, 13, 2)
  x = x.requires_grad_(True)
  assert torch.autograd.gradcheck(lambda t: po.loss_terms(t, y, 0.2, padding)[0], (x,), eps=1e-6, atol=1e-7)
  assert torch.autograd.gradcheck(lambda t: po.loss_terms(t, y, 1.0, padding)[0], (x,), eps=1e-6, atol=1e-7)


def test_known_answers():
  x, _ = po.make_pair('random', 19, 23, 3)
  # identical images: ssim 1 everywhere, zero gradient
  xg = x.clone().requires_grad_(True)
  loss, l1, ssim = po.loss_terms(xg, x.clone(), 0.2, 'same')
  loss.backward()
  assert float((po.ssim_map(x, x) - 1).abs().max()) < 1e-12 and abs(float(ssim.detach()) - 1) < 1e-12 and float(l1.detach()) == 0.0
  assert float(xg.grad.abs().max()) < 1e-12
  # constant images a, b: interior (2ab + C1) / (a^2 + b^2 + C1); borders by the partial window mass W(p):
  # mu = a W, s11 = a^2 W (1 - W), s22 = b^2 W (1 - W), s12 = a b W (1 - W)
  a, b, h, w = 0.7, 0.4, 25, 27
  m = po.ssim_map(torch.full((h, w, 1), a, dtype=torch.float64), torch.full((h, w, 1), b, dtype=torch.float64))[..., 0]
  assert float((m[5:-5, 5:-5] - (2 * a * b + po.C1) / (a * a + b * b + po.C1)).abs().max()) < 1e-12
  g = po.window()

  def mass(n):
    return torch.stack([g[max(0, 5 - p):min(11, n + 5 - p)].sum() for p in range(n)])

  W = torch.outer(mass(h), mass(w))
  v = W * (1 - W)
  want = ((2 * a * b * W * W + po.C1) * (2 * a * b * v + po.C2)
          / (((a * a + b * b) * W * W + po.C1) * ((a * a + b * b) * v + po.C2)))
  assert float((m - want).abs().max()) < 1e-12
  # valid = same cropped by 5
  y, _ = po.make_pair('random', 19, 23, 3, seed=1)
  assert float((po.ssim_map(x, y, 'valid') - po.ssim_map(x, y, 'same')[5:-5, 5:-5]).abs().max()) < 1e-12


@pytest.mark.parametrize('padding', ['same', 'valid'])
@pytest.mark.parametrize('lam', po.LAMBDAS)
def test_analytic_gradient_formula_equals_autograd(lam, padding):
  """dL/dx = (1 - lam)/N1 sign(x - y) - lam/N2 (G*A + 2 x G*B + y G*C), the formula the backward kernel implements"""
  x, y = po.make_pair('smooth_noisy', 21, 18, 3)
  xg = x.clone().requires_grad_(True)
  loss, l1, ssim = po.loss_terms(xg, y, lam, padding)
  loss.backward()
  loss, l1, ssim = loss.detach(), l1.detach(), ssim.detach()
  parts = po.analytic(x, y, padding)
  loss_a, grad_a = po.combine(parts, lam)
  assert abs(float(loss_a - loss)) < 1e-12 and abs(float(parts['l1'] - l1)) < 1e-12 and abs(float(parts['ssim'] - ssim)) < 1e-12
  assert float((grad_a - xg.grad).abs().max()) <= 1e-12


# where each mutation must show: (input kind, padding, lam) among the GPU test's inputs (KIND_SHAPE)
MUTATION_CASES = {
  'sigma_1_4': ('random', 'same', 0.2),
  'window_not_normalised': ('random', 'same', 0.2),
  'c2_c1_swapped': ('random', 'same', 0.2),
  'factor_2_dropped': ('random', 'same', 0.2),
  'c_term_uses_x': ('random', 'same', 0.2),
  'halo_clamped': ('smooth_noisy', 'same', 0.2),
  'sign_dropped': ('random', 'same', 0.2),
  'n1_for_n2': ('random', 'valid', 0.2),
}


def test_every_mutation_is_listed():
  assert set(MUTATION_CASES) == set(po.MUTATIONS)


@pytest.mark.parametrize('mutation', po.MUTATIONS)
def test_float32_tolerance_rejects_the_mutation(mutation):
  """Each mutated oracle leaves the float32 tolerance (in the gradient, and in the loss where the forward changes) on the
  named GPU test input.  (The float32 torch composition is inside it on every input by construction: the tolerance is
  four times its own deviation plus the floor; test_float32_composition_is_inside_the_tolerance states it.)"""
  kind, padding, lam = MUTATION_CASES[mutation]
  x, y = po.make_pair(kind, *po.KIND_SHAPE)
  parts = po.analytic(x, y, padding)
  tol = po.tolerances(x, y, lam, padding, parts)
  loss, grad = po.combine(parts, lam)
  loss_m, grad_m = po.combine(po.analytic(x, y, padding, mutation), lam)
  grad_excess = float((grad_m - grad).abs().max()) / tol['grad']
  loss_excess = abs(float(loss_m - loss)) / tol['loss']
  print(f"{mutation}: gradient off by {grad_excess:.1f} x tolerance, loss by {loss_excess:.1f} x")
  assert grad_excess > 1.0
  if mutation not in ('factor_2_dropped', 'c_term_uses_x', 'sign_dropped'):      # those three are gradient-only
    assert loss_excess > 1.0


@pytest.mark.parametrize('kind', po.KINDS)
def test_float32_composition_is_inside_the_tolerance(kind):
  x, y = po.make_pair(kind, *po.KIND_SHAPE)
  for padding in ('same', 'valid'):
    parts = po.analytic(x, y, padding)
    comp = {k: v.double() for k, v in po.torch_composition(x, y, padding).items()}
    for lam in po.LAMBDAS:
      tol = po.tolerances(x, y, lam, padding, parts)
      (loss, grad), (loss32, grad32) = po.combine(parts, lam), po.combine(comp, lam)
      assert abs(float(loss32 - loss)) <= tol['loss'] and float((grad32 - grad).abs().max()) <= tol['grad']
      assert all(v > 0 for v in tol.values()) or kind == 'identical'
      # the tolerance stays an error bound, not a licence: far below the quantities themselves wherever they are not ~0
      if kind != 'identical':
        assert tol['grad'] < 2e-2 * float(grad.abs().max()) or lam == 0.0


def test_abi_declares_and_checks_the_photometric_entry_points(lib):
  from tests.test_abi import declared_functions
  assert {'ms_photometric_fwd', 'ms_photometric_bwd'} <= set(declared_functions())
  assert re.search(r'#define MS_VERSION (\d+)', (_lib.CSRC_DIR.parent.parent / 'include' / 'mi355_splat.h').read_text()).group(1) == '501'
  n = ctypes.c_size_t(0)

  def fwd(h=64, w=64, c=3, dtype=_lib.MS_F32, pad=_lib.PAD_SAME, lam=0.2, image=None, tmp=None, out=None, tmp_bytes=n):
    return lib.ms_photometric_fwd(image, image, h, w, c, dtype, pad, lam, None, None, None, tmp,
                                  ctypes.byref(tmp_bytes) if tmp_bytes is not None else None, out, None)

  # scratch query: one pair of doubles per workgroup (float: 32-row tiles of 64 floats, double: 16-row tiles)
  assert fwd(2048, 2048, 3) == 0 and n.value >= 16 * (2048 // 32) * (2048 * 3 // 64)
  small = n.value
  assert fwd(2048, 2048, 3, dtype=_lib.MS_F64) == 0 and n.value >= 2 * small
  assert fwd(1, 1, 1) == 0 and 16 <= n.value <= 256
  assert fwd(11, 11, 4, pad=_lib.PAD_VALID) == 0
  # argument errors (all before any launch)
  assert fwd(c=5) == -1 and b'C' in lib.ms_last_error_string()
  assert fwd(c=0) == -1 and fwd(h=0) == -1 and fwd(w=-3) == -1
  assert fwd(10, 64, 3, pad=_lib.PAD_VALID) == -1 and b'valid' in lib.ms_last_error_string()
  assert fwd(64, 10, 3, pad=_lib.PAD_VALID) == -1
  assert fwd(pad=7) == -1 and fwd(lam=1.5) == -1
  assert fwd(dtype=9) == -2
  assert fwd(tmp_bytes=None) == -1
  big = ctypes.c_size_t(1 << 20)
  assert fwd(image=None, tmp=1, out=1, tmp_bytes=big) == -1 and b'null' in lib.ms_last_error_string()
  assert fwd(image=1, tmp=1, out=None, tmp_bytes=big) == -1
  assert fwd(image=1, tmp=1, out=1, tmp_bytes=ctypes.c_size_t(8)) == -3
  assert lib.ms_photometric_fwd(1, 1, 64, 64, 3, 0, 0, 0.2, 1, None, None, 1, ctypes.byref(big), 1, None) == -1   # one map of three

  def bwd(h=64, w=64, c=3, dtype=_lib.MS_F32, pad=_lib.PAD_SAME, go=1, grad=1):
    return lib.ms_photometric_bwd(1, 1, 1, 1, 1, go, h, w, c, dtype, pad, 0.2, grad, None)

  assert bwd(c=5) == -1 and bwd(h=0) == -1 and bwd(10, 10, 3, pad=_lib.PAD_VALID) == -1
  assert bwd(dtype=9) == -2
  assert bwd(go=None) == -1 and bwd(grad=None) == -1


def test_python_interface_refuses_without_a_gpu():
  from taichi_splatting_amd import l1_ssim_loss, ssim
  x = torch.zeros((16, 16, 3))
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    l1_ssim_loss(x, x)
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    ssim(x, x)
