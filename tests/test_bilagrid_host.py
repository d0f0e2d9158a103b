"""No GPU: the two float64 oracles of the bilateral-grid slice (tests/bilagrid_oracle.py) agree and pass gradcheck, the
torch parts of taichi_splatting_amd/appearance.py do what they say, and the C-ABI of csrc/bilagrid.hip and the Python
entry point answer their argument checks."""
import ctypes

import pytest
import torch

from taichi_splatting_amd import _lib
from tests import bilagrid_oracle as bo

ORACLE_SHAPES = [(5, 7, 8, 16, 16), (9, 6, 2, 2, 2), (4, 4, 3, 1, 5), (6, 5, 1, 3, 2)]


@pytest.mark.parametrize('shape', ORACLE_SHAPES)
def test_the_two_oracles_agree(shape):
  image, grid, grad_out = bo.make_case(*shape)
  lum = bo.luminance(image)
  assert bool((lum < 0).any()) and bool((lum > 1).any())           # both sides of the clamp take part
  out_a, gi_a, gg_a = bo.reference(image, grid, grad_out)
  out_b, gi_b, gg_b = bo.slice_loop(image, grid, grad_out)
  assert float((out_a - out_b).abs().max()) < 1e-12
  assert float((gi_a - gi_b).abs().max()) < 1e-12
  assert float((gg_a - gg_b).abs().max()) < 1e-12


def test_oracle_passes_gradcheck():
  image, grid, _ = bo.make_case(9, 6, 2, 2, 2)
  image = image * 0.5 + 0.25                 # keep the finite differences off the luminance clamp's two kinks
  assert torch.autograd.gradcheck(bo.slice_grid_sample, (image.requires_grad_(True), grid.requires_grad_(True)),
                                  eps=1e-6, atol=1e-7)


def test_oracle_of_the_identity_grid_is_the_image():
  from taichi_splatting_amd import identity_bilateral_grid
  image, _, _ = bo.make_case(7, 9, 4, 3, 5)
  grid = identity_bilateral_grid(4, 3, 5, dtype=torch.float64)
  assert grid.shape == (12, 4, 3, 5) and grid.is_contiguous()
  assert float((bo.slice_grid_sample(image, grid) - image).abs().max()) < 1e-14
  with pytest.raises(ValueError):
    identity_bilateral_grid(0, 3, 5)


def test_total_variation():
  from taichi_splatting_amd import bilateral_grid_tv, BilateralGrids
  gen = torch.Generator().manual_seed(3)
  g = torch.randn((2, 12, 4, 3, 5), generator=gen, dtype=torch.float64)
  want = (((g[:, :, 1:] - g[:, :, :-1]) ** 2).mean() + ((g[:, :, :, 1:] - g[:, :, :, :-1]) ** 2).mean()
          + ((g[..., 1:] - g[..., :-1]) ** 2).mean())
  assert abs(float(bilateral_grid_tv(g) - want)) < 1e-14
  assert abs(float(bilateral_grid_tv(g[0]) - bilateral_grid_tv(g[:1]))) < 1e-14       # one grid without the leading axis
  # size-1 axes contribute 0: only the remaining axes count, and a single vertex has no variation at all
  flat = torch.randn((12, 1, 3, 1), generator=gen, dtype=torch.float64)
  assert abs(float(bilateral_grid_tv(flat) - ((flat[:, :, 1:] - flat[:, :, :-1]) ** 2).mean())) < 1e-14
  assert float(bilateral_grid_tv(torch.randn((12, 1, 1, 1), generator=gen))) == 0.0
  assert float(bilateral_grid_tv(BilateralGrids(3).grids.detach())) == 0.0
  assert float(BilateralGrids(2, (4, 1, 2)).tv_loss().detach()) == 0.0
  g.requires_grad_(True)
  bilateral_grid_tv(g).backward()
  assert g.grad is not None and float(g.grad.abs().max()) > 0
  with pytest.raises(ValueError):
    bilateral_grid_tv(torch.zeros((11, 2, 2, 2)))


def test_bilateral_grids_module():
  from taichi_splatting_amd import BilateralGrids
  m = BilateralGrids(5)
  assert [n for n, _ in m.named_parameters()] == ['grids']
  assert m.grids.shape == (5, 12, 8, 16, 16) and m.grids.dtype == torch.float32 and m.grids.requires_grad
  m = BilateralGrids(2, grid_shape=(5, 3, 4), dtype=torch.float64)                    # (Gx, Gy, L)
  assert m.grids.shape == (2, 12, 4, 3, 5)
  eye = torch.eye(3, 4, dtype=torch.float64).reshape(1, 12, 1, 1, 1)
  assert bool((m.grids == eye).all())
  for bad in ((0, 3, 4), (5, 129, 4), (5, 3, 17)):
    with pytest.raises(ValueError):
      BilateralGrids(2, grid_shape=bad)
  with pytest.raises(ValueError):
    BilateralGrids(0)
  image = torch.zeros((4, 4, 3), dtype=torch.float64)
  with pytest.raises(IndexError):
    m(image, 2)
  with pytest.raises(TypeError):
    m(image, torch.tensor(0.0))
  with pytest.raises(TypeError):
    m(image, torch.tensor([0]))


def test_exports():
  import taichi_splatting_amd as pkg
  from taichi_splatting_amd import appearance
  for name in ('apply_bilateral_grid', 'BilateralGrids', 'identity_bilateral_grid', 'bilateral_grid_tv'):
    assert name in pkg.__all__ and getattr(pkg, name) is getattr(appearance, name)
  import importlib
  assert hasattr(importlib.import_module('taichi_splatting_amd.examples.fit_appearance'), 'main')


def test_python_interface_checks_its_arguments():
  from taichi_splatting_amd import apply_bilateral_grid
  image, grid = torch.zeros((8, 9, 3)), torch.zeros((12, 4, 3, 5))
  for bad_image in (torch.zeros((8, 9, 4)), torch.zeros((8, 9)), torch.zeros((3, 8, 9, 3)), torch.zeros((0, 9, 3))):
    with pytest.raises(ValueError):
      apply_bilateral_grid(bad_image, grid)
  for bad_grid in (torch.zeros((11, 4, 3, 5)), torch.zeros((12, 3, 5)), torch.zeros((12, 17, 3, 5)), torch.zeros((12, 4, 129, 5)),
                   torch.zeros((12, 4, 3, 129)), torch.zeros((12, 0, 3, 5))):
    with pytest.raises(ValueError):
      apply_bilateral_grid(image, bad_grid)
  with pytest.raises(TypeError):
    apply_bilateral_grid(image, grid.double())
  with pytest.raises(TypeError):
    apply_bilateral_grid(image.half(), grid.half())
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    apply_bilateral_grid(image, grid)


def footprint_chunks(n, G):
  """64-pixel chunks of the widest vertex footprint along an axis: bg_range / bg_extent of csrc/bilagrid.hip"""
  if G == 1:
    return -(-n // 64)
  slack, widest = 1 + (n >> 20), 0
  for v in range(G):
    a, b = max(v - 1, 0) * n // (G - 1), (v + 1) * n // (G - 1)
    widest = max(widest, min(n, b + 1 + slack) - max(0, a - slack))
  return -(-widest // 64)


def test_abi_declares_and_checks_the_bilagrid_entry_points(lib):
  from tests.test_abi import declared_functions
  assert {'ms_bilagrid_fwd', 'ms_bilagrid_bwd'} <= set(declared_functions())
  assert lib.ms_version() == 501

  def fwd(h=64, w=64, l=8, gy=16, gx=16, dtype=_lib.MS_F32, image=1, grid=1, out=1):
    return lib.ms_bilagrid_fwd(image, grid, h, w, l, gy, gx, dtype, out, None)

  # (every check comes before any launch: the pointers are never read)
  assert fwd(image=None) == -1 and b'null' in lib.ms_last_error_string()
  assert fwd(grid=None) == -1 and fwd(out=None) == -1
  assert fwd(h=0) == -1 and fwd(w=-2) == -1 and fwd(l=0) == -1 and fwd(gy=0) == -1 and fwd(gx=-1) == -1
  assert fwd(dtype=9) == -2 and b'dtype' in lib.ms_last_error_string()
  assert fwd(l=17) == -2 and fwd(gy=129) == -2 and fwd(gx=129) == -2
  assert fwd(h=40000, w=40000) == -2 and b'too large' in lib.ms_last_error_string()

  n = ctypes.c_size_t(0)
  big = ctypes.c_size_t(1 << 30)

  def bwd(h=64, w=64, l=8, gy=16, gx=16, dtype=_lib.MS_F32, image=1, grid=1, go=1, gi=1, gg=1, tmp=1, tmp_bytes=big):
    return lib.ms_bilagrid_bwd(image, grid, go, h, w, l, gy, gx, dtype, gi, gg, tmp,
                               ctypes.byref(tmp_bytes) if tmp_bytes is not None else None, None)

  def query(h, w, l, gy, gx):
    assert bwd(h, w, l, gy, gx, image=None, grid=None, go=None, gi=None, gg=None, tmp=None, tmp_bytes=n) == 0
    return n.value

  # scratch query: (L, 12) doubles per (vertex, 64 x 64 chunk of the widest footprint), rounded up to 256 bytes
  for h, w, l, gy, gx in ((2048, 2048, 8, 16, 16), (37, 53, 8, 16, 16), (1, 1, 1, 1, 1), (130, 70, 2, 2, 2), (300, 4096, 16, 1, 128)):
    chunks = footprint_chunks(w, gx) * footprint_chunks(h, gy)
    want = chunks * gy * gx * l * 12 * 8
    assert query(h, w, l, gy, gx) == -(-want // 256) * 256, (h, w, l, gy, gx)
  assert query(2048, 2048, 8, 16, 16) == 25 * 256 * 96 * 8
  assert query(130, 70, 2, 2, 2) == 3 * 2 * 4 * 24 * 8              # a multi-chunk reduction: 6 chunks per vertex

  assert bwd(tmp_bytes=None) == -1
  assert bwd(image=None) == -1 and b'null' in lib.ms_last_error_string()
  assert bwd(grid=None) == -1 and bwd(go=None) == -1
  assert bwd(gi=None, gg=None) == -1 and b'both' in lib.ms_last_error_string()
  assert bwd(h=0) == -1 and bwd(w=0) == -1 and bwd(l=-1) == -1 and bwd(gy=0) == -1 and bwd(gx=0) == -1
  assert bwd(dtype=2) == -2 and bwd(l=17) == -2 and bwd(gy=200) == -2 and bwd(gx=129) == -2
  assert bwd(tmp_bytes=ctypes.c_size_t(8)) == -3 and b'tmp_bytes' in lib.ms_last_error_string()
  with pytest.raises(ValueError):
    _lib.check(-3, "bilagrid")
