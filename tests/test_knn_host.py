"""k nearest neighbours without a GPU: the float64 oracle against answers worked by hand, the argument checks and the
scratch query of ms_knn_points (they run before any launch), and the Python operators' refusals."""
import ctypes
import math
import re
from pathlib import Path

import pytest
import torch

from taichi_splatting_amd import Gaussians3D, _lib
from tests import knn_oracle

HEADER = Path(__file__).resolve().parent.parent / 'include' / 'mi355_splat.h'
FAKE = 256          # a non-null "pointer": every call below returns before anything is read through it


# ---- the oracle -------------------------------------------------------------------------------------------------------
def test_oracle_on_a_unit_lattice():
  g = torch.stack(torch.meshgrid(*(torch.arange(5, dtype=torch.float32),) * 3, indexing='ij'), dim=-1).reshape(-1, 3)
  d2, idx = knn_oracle.brute_force(g, 3, chunk=7)
  interior, corner = 2 * 25 + 2 * 5 + 2, 0
  assert d2[interior].tolist() == [1.0, 1.0, 1.0] and d2[corner].tolist() == [1.0, 1.0, 1.0]
  assert sorted(idx[corner].tolist()) == [1, 5, 25]           # the three axis neighbours of (0, 0, 0)
  assert all((g[j] - g[interior]).abs().sum() == 1 for j in idx[interior].tolist())
  d6, _ = knn_oracle.brute_force(g, 7)
  assert d6[interior].tolist() == [1.0] * 6 + [2.0] and d6[corner].tolist() == [1.0] * 3 + [2.0] * 3 + [3.0]
  assert (idx != torch.arange(125)[:, None]).all()


def test_oracle_on_coincident_and_too_few_points():
  p = torch.tensor([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [4.0, 6.0, 3.0]])
  d2, idx = knn_oracle.brute_force(p, 2)
  assert d2.tolist() == [[0.0, 25.0], [0.0, 25.0], [25.0, 25.0]]
  assert idx[0].tolist() == [1, 2] and idx[1].tolist() == [0, 2] and sorted(idx[2].tolist()) == [0, 1]
  d2, idx = knn_oracle.brute_force(p[1:], 3)                  # N = 2, k = 3: one finite entry
  assert d2.tolist() == [[25.0, math.inf, math.inf]] * 2 and idx.tolist() == [[1, -1, -1], [0, -1, -1]]
  d2, idx = knn_oracle.brute_force(p[:1], 3)
  assert d2.tolist() == [[math.inf] * 3] and idx.tolist() == [[-1] * 3]


def test_oracle_uses_differences_not_the_expanded_form():
  """two points 2^-10 apart at 10^4: the expanded form in float32 returns 0 or garbage; the oracle the exact value"""
  p = torch.tensor([[1.0e4, 0.0, 0.0], [1.0e4 + 2.0 ** -10, 0.0, 0.0]])
  d2, _ = knn_oracle.brute_force(p, 1)
  assert d2.tolist() == [[2.0 ** -20]] * 2
  assert knn_oracle.kernel_dist2_f32(p.numpy(), [0], [1]).tolist() == [2.0 ** -20]


def test_criterion_accepts_the_float32_expression_and_rejects_wrong_answers():
  p = knn_oracle.make('uniform_cube', 300, 256)
  want, idx = knn_oracle.brute_force(p, 8)
  rows = torch.arange(300)[:, None].expand(300, 3)
  got = torch.from_numpy(knn_oracle.kernel_dist2_f32(p.numpy(), rows.numpy(), idx[:, :3].numpy()))
  got, perm = torch.sort(got, dim=1)
  index = torch.gather(idx[:, :3], 1, perm).to(torch.int32)
  assert knn_oracle.check(p, 3, got, index, want) <= 4.0
  with pytest.raises(AssertionError, match="relative error"):
    knn_oracle.check(p, 3, got * (1 + 2.0 ** -20), None, want)
  with pytest.raises(AssertionError, match="own neighbour"):
    bad = index.clone()
    bad[7, 0] = 7
    knn_oracle.check(p, 3, got, bad, want)
  with pytest.raises(AssertionError, match="bitwise"):
    bad = index.clone()
    bad[7, 0] = index[8, 0] if index[8, 0] not in index[7] and index[8, 0] != 7 else index[9, 0]
    knn_oracle.check(p, 3, got, bad, want)
  with pytest.raises(AssertionError):
    knn_oracle.check(p, 3, want[:, 1:4].float(), None, want)     # the second to fourth nearest


# ---- the C entry point ------------------------------------------------------------------------------------------------
def _call(lib, points=FAKE, order=FAKE, n=1000, k=3, out=FAKE, index=None, stats=None, tmp=FAKE, nbytes=1 << 40):
  size = None if nbytes is None else ctypes.c_size_t(nbytes)
  rc = lib.ms_knn_points(points, order, n, k, out, index, stats, tmp, None if size is None else ctypes.byref(size), None)
  return rc, lib.ms_last_error_string(), (None if size is None else size.value)


def test_knn_points_is_declared_bound_and_sized_like_the_header(lib):
  assert hasattr(lib, 'ms_knn_points') and 'ms_knn_points' in _lib.SIGNATURES
  from taichi_splatting_amd.misc.knn import BLOCK      # (misc.knn the attribute is the function, not the module)
  block = int(re.search(r'#define MS_KNN_BLOCK (\d+)', HEADER.read_text()).group(1))
  assert block == _lib.KNN_BLOCK == BLOCK
  assert lib.ms_version() == 501              # an addition within the ABI generation


def test_knn_points_argument_errors_name_the_argument(lib):
  for kw, word in ((dict(n=-1), b'n < 0'), (dict(n=1 << 31), b'n >= 2^31'), (dict(n=1 << 40), b'n >= 2^31'),
                   (dict(k=0), b'k must'), (dict(k=9), b'k must'), (dict(k=-3), b'k must'),
                   (dict(points=None), b'points3'), (dict(order=None), b'order'), (dict(out=None), b'out_dist2'),
                   (dict(nbytes=None), b'tmp_bytes'), (dict(nbytes=None, tmp=None), b'tmp_bytes')):
    rc, text, _ = _call(lib, **kw)
    assert rc == -1, (kw, rc, text)           # MS_ERR_BAD_ARG
    assert text.startswith(b'ms_knn_points') and word in text, (kw, text)
  with pytest.raises(ValueError, match="k must"):
    _lib.check(_call(lib, k=12)[0], "knn")


def test_knn_points_scratch_query_and_too_small_scratch(lib):
  sizes = []
  for n in (0, 1, 2, 255, 256, 257, 1000, 65536, 65537, 6_000_000, (1 << 31) - 1):
    rc, _, size = _call(lib, points=None, order=None, out=None, n=n, tmp=None, nbytes=12345)
    assert rc == 0
    sizes.append(size)
    blocks = (n + _lib.KNN_BLOCK - 1) // _lib.KNN_BLOCK
    assert size >= 16 * n + 32 * blocks          # a 16-byte row per point, two 16-byte box corners per block
  assert sizes == sorted(sizes) and sizes[0] < sizes[3] < sizes[-1], sizes      # monotone in n
  need = sizes[6]
  rc, text, _ = _call(lib, n=1000, nbytes=need - 1)
  assert rc == -1 and b'tmp_bytes too small' in text
  # the size is checked before the pointers, as in ms_radix_sort_pairs: a query never needs them
  rc, text, _ = _call(lib, points=None, n=1000, nbytes=need)
  assert rc == -1 and b'points3' in text


def test_knn_points_with_no_points_returns_without_a_launch(lib):
  rc, _, _ = _call(lib, points=None, order=None, out=None, n=0, nbytes=0)
  assert rc == 0


# ---- the Python operators ---------------------------------------------------------------------------------------------
def test_operators_have_no_cpu_fallback():
  from taichi_splatting_amd.misc import knn, mean_knn_dist2
  from taichi_splatting_amd.misc.knn import morton_order
  p = torch.rand((10, 3))
  for call in (lambda: knn(p), lambda: knn(p, 1, return_indices=False), lambda: mean_knn_dist2(p), lambda: morton_order(p),
               lambda: Gaussians3D.from_point_cloud(p), lambda: Gaussians3D.from_point_cloud(p, torch.rand((10, 3)), sh_degree=3)):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
      call()


def test_operator_argument_errors():
  from taichi_splatting_amd.misc import knn, mean_knn_dist2
  p = torch.rand((10, 3))
  for bad in (lambda: knn(p, 0), lambda: knn(p, 9), lambda: knn(p, 2.0), lambda: knn(torch.rand((10, 2))),
              lambda: knn(torch.rand((10,))), lambda: mean_knn_dist2(p[:1]), lambda: mean_knn_dist2(p[:0]),
              lambda: mean_knn_dist2(p, 0)):
    with pytest.raises(ValueError):
      bad()


def test_from_point_cloud_argument_errors():
  p, c = torch.rand((10, 3)), torch.rand((10, 3))
  f = Gaussians3D.from_point_cloud
  for bad, word in ((lambda: f(torch.rand((10, 4))), "points"), (lambda: f(p[:1]), "at least 2"),
                    (lambda: f(p, c[:9]), "colours"), (lambda: f(p, torch.rand((10, 4))), "colours"),
                    (lambda: f(p, c, sh_degree=4), "sh_degree"), (lambda: f(p, c, sh_degree=-1), "sh_degree"),
                    (lambda: f(p, c, sh_degree=1.0), "sh_degree"), (lambda: f(p, k=0), "k must"), (lambda: f(p, k=9), "k must"),
                    (lambda: f(p, initial_alpha=0.0), "initial_alpha"), (lambda: f(p, initial_alpha=1.0), "initial_alpha"),
                    (lambda: f(p, min_dist2=0.0), "min_dist2"), (lambda: f(p, min_dist2=-1.0), "min_dist2")):
    with pytest.raises(ValueError, match=word):
      bad()


def test_install_as_taichi_splatting_carries_the_new_names():
  import sys
  import taichi_splatting_amd
  taichi_splatting_amd.install_as_taichi_splatting()
  assert sys.modules['taichi_splatting.misc.knn'].knn is sys.modules['taichi_splatting_amd.misc.knn'].knn
  assert hasattr(sys.modules['taichi_splatting'].Gaussians3D, 'from_point_cloud')
