"""Fixed-budget densification without a GPU: the oracle (tests/relocate_oracle.py) against hand-computed cases, argument
validation of the Python entry points, the CPU-tensor refusal and the new C-ABI symbols."""
import ctypes
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from taichi_splatting_amd import _lib
from tests import relocate_oracle as oracle

HEADER = Path(__file__).resolve().parent.parent / 'include' / 'mi355_splat.h'
SYMBOLS = ('ms_relocate_weights', 'ms_relocate_draw', 'ms_relocate_fresh', 'ms_relocate_move', 'ms_perturb_positions')


# ---- the oracle against hand-computed cases ---------------------------------------------------------------------------

@pytest.mark.parametrize('o', [0.5, 0.75, 0.99, 1 - 2.0 ** -20])
def test_ratio_one_changes_nothing_exactly(o):
  """1 - (1 - o)^1 is o exactly where 1 - o is exact, which (Sterbenz) is every o in [0.5, 1]; denom is then o' alone."""
  new, coeff = oracle.opacity_and_coeff(o, 1)
  assert new == o and coeff == 1.0


@pytest.mark.parametrize('o', [0.006, 0.1, 0.3])
def test_ratio_one_below_a_half_is_one_rounding_away(o):
  new, coeff = oracle.opacity_and_coeff(o, 1)
  assert abs(new - o) <= np.spacing(1.0) and abs(coeff - 1.0) <= 2 * np.spacing(1.0) / o


def test_hand_computed_coefficients():
  new, coeff = oracle.opacity_and_coeff(0.5, 2)
  assert new == pytest.approx(1 - math.sqrt(0.5), rel=1e-15)
  # denom = 2 o' - o'^2 / sqrt(2)
  assert coeff == pytest.approx(0.5 / (2 * new - new * new / math.sqrt(2)), rel=1e-15)
  assert coeff == pytest.approx(0.9521519537657248, rel=1e-13)
  new, coeff = oracle.opacity_and_coeff(0.99, 51)
  assert new == pytest.approx(1 - 0.01 ** (1 / 51), rel=1e-15)
  assert coeff == pytest.approx(0.6421244069737009, rel=1e-12)


def test_the_kernel_form_of_the_double_sum_is_the_same_number():
  """csrc/relocate.hip sums over k alone: the inner sum over i is C(ratio, k + 1) (hockey-stick identity), which it
  takes as two neighbours of row ratio - 1 of the 51 x 51 table (Pascal's rule; exact integers).  The same value as the
  literal double sum, to the rounding of float64."""
  from taichi_splatting_amd.optim.relocate import binomial_table
  table = binomial_table()
  assert len(table) == 51 and table[50][25] == float(math.comb(50, 25)) and table[3][5] == 0.0
  assert max(max(row) for row in table) < 2.0 ** 53
  for o, ratio in ((0.006, 2), (0.5, 7), (0.99, 51), (1 - 6e-8, 51), (0.3, 51)):
    new, coeff = oracle.opacity_and_coeff(o, ratio)
    denom, p = 0.0, 1.0
    for k in range(ratio):
      p *= new
      column = table[ratio - 1][k] + (table[ratio - 1][k + 1] if k + 1 < 51 else 0.0)
      assert column == sum(table[m][k] for m in range(k, ratio))
      assert column == math.comb(ratio, k + 1)
      denom += (-1.0) ** k * p / math.sqrt(k + 1) * column
    assert o / denom == pytest.approx(coeff, rel=1e-9)


def test_weights_threshold_and_draw_by_hand():
  t = oracle.threshold(0.005)
  assert t == np.float32(math.log(0.005 / 0.995)) and t.dtype == np.float32
  a = np.array([0.0, float(t), np.nextafter(t, np.float32(0)), np.nan, -100.0, 40.0, -5.0], dtype=np.float32)
  assert oracle.dead_rows(a, 0.005).tolist() == [False, True, False, True, True, False, False]
  w = oracle.weights(a, 0.005)
  assert w[0] == 1 << 23 and w[1] == 0 and w[3] == 0 and w[4] == 0 and w[5] == 1 << 24
  assert w[6] == round(2 ** 24 / (1 + math.exp(5.0)))
  # a weight never rounds to zero for a live row
  assert oracle.weights(np.array([-20.0], dtype=np.float32), 1e-12)[0] == 1

  # cdf = [2, 2, 5, 5]: targets 0, 1 -> row 0; 2, 3, 4 -> row 2
  weight = [2, 0, 3, 0]
  top = 1 << 64
  src, count, total = oracle.draw(weight, [0, (2 * top) // 5 - 1, 0, top - 1])
  assert total == 5 and src.tolist() == [0, 0, 2, 2] and count.tolist() == [1, 0, 1, 0]
  src, count, _ = oracle.draw(weight, [0, (2 * top + 4) // 5, 0, 0])     # target exactly 2: the first cdf > 2 is row 2
  assert src.tolist() == [0, 2, 2, 0] and count.tolist() == [1, 0, 1, 0]
  src, count, total = oracle.draw([0, 0, 0], [5, 6, 7])                  # every row dead: nothing moves
  assert total == 0 and src.tolist() == [0, 1, 2] and count.tolist() == [0, 0, 0]


def test_perturbation_by_hand():
  """An identity rotation (scaled: the quaternion is normalised first) and scales (1, 2, 3): Sigma = diag(1, 4, 9)."""
  ls = np.log(np.array([[1.0, 2.0, 3.0]]))
  delta, g, smax = oracle.perturbation(ls, np.array([[0.0, 0.0, 0.0, 2.5]]), np.array([-40.0]), np.array([[1.0, 1.0, -1.0]]), 0.5)
  want_g = 1.0 / (1.0 + math.exp(-100.0 * 0.005))
  assert g[0] == pytest.approx(want_g, rel=1e-12) and smax[0] == pytest.approx(9.0, rel=1e-14)
  assert delta[0] == pytest.approx(0.5 * want_g * np.array([1.0, 4.0, -9.0]), rel=1e-12)
  # a quarter turn about z swaps the x and y axes of the covariance
  s = math.sqrt(0.5)
  delta, _, _ = oracle.perturbation(ls, np.array([[0.0, 0.0, s, s]]), np.array([-40.0]), np.array([[1.0, 0.0, 0.0]]), 1.0)
  assert delta[0] == pytest.approx(want_g * np.array([4.0, 0.0, 0.0]), rel=1e-12, abs=1e-15)
  # an opaque gaussian does not move
  _, g, _ = oracle.perturbation(ls, np.array([[0.0, 0.0, 0.0, 1.0]]), np.array([10.0]), np.zeros((1, 3)), 1.0)
  assert g[0] < 1e-40


# ---- argument validation and the CPU refusal --------------------------------------------------------------------------

def cpu_params(n=8):
  from taichi_splatting_amd.optim import ParameterClass
  tensors = dict(position=torch.randn(n, 3), log_scaling=torch.randn(n, 3), rotation=torch.randn(n, 4),
                 alpha_logit=torch.randn(n, 1), feature=torch.randn(n, 3, 16))
  return ParameterClass(tensors, {k: dict(lr=0.01) for k in tensors}, optimizer=torch.optim.Adam)


def cpu_gaussians(n=8):
  from taichi_splatting_amd import Gaussians3D
  return Gaussians3D(position=torch.randn(n, 3), log_scaling=torch.randn(n, 3), rotation=torch.randn(n, 4),
                     alpha_logit=torch.randn(n, 1), feature=torch.randn(n, 3, 16), batch_size=[n])


def test_argument_validation():
  from taichi_splatting_amd import perturb_positions, relocate, relocate_gaussians3d
  from taichi_splatting_amd.optim.relocate import logit_threshold
  assert logit_threshold(0.005) == float(oracle.threshold(0.005))
  params, g = cpu_params(), cpu_gaussians()
  for bad in (0.0, -0.1, 1.0, 1.5, float('nan')):
    with pytest.raises(ValueError, match="min_opacity"):
      relocate(params, min_opacity=bad)
    with pytest.raises(ValueError, match="min_opacity"):
      relocate_gaussians3d(g, min_opacity=bad)
  for bad in (torch.zeros(8, dtype=torch.int32), torch.zeros(7, dtype=torch.int64), torch.zeros(8, 1, dtype=torch.int64)):
    with pytest.raises(ValueError, match="random"):
      params.relocate(random=bad)
    with pytest.raises(ValueError, match="random"):
      relocate_gaussians3d(g, random=bad)
  with pytest.raises(KeyError, match="opacity_logit"):
    relocate(params, opacity='opacity_logit')
  with pytest.raises(KeyError, match="scales"):
    relocate(params, scale='scales')
  for bad in (torch.zeros(8, 3, dtype=torch.float64), torch.zeros(8, 2), torch.zeros(7, 3)):
    with pytest.raises(ValueError, match="z must be"):
      perturb_positions(g, 0.1, z=bad)
  for kw in (dict(step=float('nan')), dict(step=0.1, k=float('inf')), dict(step=0.1, x0=float('nan'))):
    with pytest.raises(ValueError, match="finite"):
      perturb_positions(g, **kw)
  learnt = cpu_gaussians().requires_grad_(True)
  with pytest.raises(RuntimeError, match="require grad"):
    relocate_gaussians3d(learnt)
  with pytest.raises(RuntimeError, match="require grad"):
    perturb_positions(learnt, 0.1)


def test_cpu_tensors_are_refused():
  from taichi_splatting_amd import perturb_positions, relocate_gaussians3d
  params, g = cpu_params(), cpu_gaussians()
  before = {k: v.detach().clone() for k, v in params.tensors.items()}
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    params.relocate()
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    relocate_gaussians3d(g)
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    perturb_positions(g, 0.1)
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    perturb_positions(params, 0.1, z=torch.zeros(8, 3))
  for k, v in params.tensors.items():
    assert torch.equal(v.detach(), before[k])


# ---- the C-ABI --------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_exported_and_bound(lib):
  text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
  declared = set(re.findall(r'\b(ms_[a-z0-9_]+)\s*\(', text))
  for name in SYMBOLS:
    assert name in declared, f"{name} is not declared in mi355_splat.h"
    assert hasattr(lib, name), f"{name} is not exported"
    assert name in _lib.SIGNATURES
  assert int(re.search(r'#define MS_RELOCATE_MAX_RATIO (\d+)', text).group(1)) == _lib.RELOCATE_MAX_RATIO == oracle.MAX_RATIO


def test_descriptor_layout_matches_the_header(tmp_path):
  src = tmp_path / 'sizes.c'
  src.write_text("""
    #include <stdio.h>
    #include <stddef.h>
    #include "mi355_splat.h"
    int main(void) {
      printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(ms_relocate_array), offsetof(ms_relocate_array, struct_size),
             offsetof(ms_relocate_array, role), offsetof(ms_relocate_array, data), offsetof(ms_relocate_array, fresh),
             offsetof(ms_relocate_array, row_bytes));
      printf("%d %d %d %d %d\\n", MS_RELOCATE_COPY, MS_RELOCATE_ZERO_TOUCHED, MS_RELOCATE_INHERIT, MS_RELOCATE_OPACITY,
             MS_RELOCATE_SCALE);
      return 0;
    }
  """)
  exe = tmp_path / 'sizes'
  subprocess.run(['gcc', '-std=c99', '-I', str(HEADER.parent), str(src), '-o', str(exe)], check=True)
  sizes, roles = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
  c = _lib.RelocateArrayC
  assert [int(x) for x in sizes.split()] == [ctypes.sizeof(c), c.struct_size.offset, c.role.offset, c.data.offset,
                                             c.fresh.offset, c.row_bytes.offset]
  assert [int(x) for x in roles.split()] == [_lib.RELOCATE_COPY, _lib.RELOCATE_ZERO_TOUCHED, _lib.RELOCATE_INHERIT,
                                             _lib.RELOCATE_OPACITY, _lib.RELOCATE_SCALE]


def descriptor(**kw):
  args = dict(struct_size=ctypes.sizeof(_lib.RelocateArrayC), role=_lib.RELOCATE_COPY, data=64, fresh=None, row_bytes=16)
  args.update(kw)
  return (_lib.RelocateArrayC * 1)(_lib.RelocateArrayC(**args))


def test_argument_errors_come_before_any_launch(lib):
  """Host-side checks only (no GPU here: a launch would fail with a HIP error, not with MS_ERR_BAD_ARG = -1)."""
  assert lib.ms_relocate_move(descriptor(), 1, 64, 64, -1, None) == -1
  assert lib.ms_relocate_move(descriptor(), 1, 64, 64, 1 << 30, None) == -1
  assert b'2^30' in lib.ms_last_error_string()
  assert lib.ms_relocate_move(descriptor(struct_size=16), 1, 64, 64, 10, None) == -4
  assert b'ABI' in lib.ms_last_error_string()
  for bad in (0, 6, -4, (1 << 20) + 4):
    assert lib.ms_relocate_move(descriptor(row_bytes=bad), 1, 64, 64, 10, None) == -1
    assert b'row_bytes' in lib.ms_last_error_string()
  for bad in (-1, 5):
    assert lib.ms_relocate_move(descriptor(role=bad), 1, 64, 64, 10, None) == -1
    assert b'role' in lib.ms_last_error_string()
  assert lib.ms_relocate_move(descriptor(data=None), 1, 64, 64, 10, None) == -1
  assert lib.ms_relocate_move(descriptor(data=66), 1, 64, 64, 10, None) == -1
  assert b'aligned' in lib.ms_last_error_string()
  assert lib.ms_relocate_move(descriptor(role=_lib.RELOCATE_OPACITY), 1, 64, 64, 10, None) == -1       # no side buffer
  assert lib.ms_relocate_move(descriptor(role=_lib.RELOCATE_SCALE, fresh=64), 1, 64, 64, 10, None) == -1
  assert b'side buffer' in lib.ms_last_error_string()
  assert lib.ms_relocate_move(descriptor(), 1, None, None, 10, None) == -1
  assert lib.ms_relocate_move(descriptor(), 1, 64, 64, 0, None) == 0            # nothing to do: no launch
  assert lib.ms_relocate_move(None, 0, 64, 64, 10, None) == 0

  assert lib.ms_relocate_weights(64, -1, 0.0, 64, 64, 64, None) == -1
  assert lib.ms_relocate_weights(64, 10, 0.0, 64, 64, None, None) == -1
  assert lib.ms_relocate_weights(64, 10, float('nan'), 64, 64, 64, None) == -1
  assert lib.ms_relocate_weights(64, 10, 0.0, 68, 64, 64, None) == -1          # int64 weights on a 4-byte boundary
  assert lib.ms_relocate_draw(64, 64, 64, -1, 64, 64, 64, None) == -1
  assert lib.ms_relocate_draw(64, None, 64, 10, 64, 64, 64, None) == -1
  assert lib.ms_relocate_draw(None, None, None, 0, None, None, None, None) == 0
  for dims in (0, 17):
    assert lib.ms_relocate_fresh(64, 64, dims, 64, 10, 0.005, 64, 64, 64, 64, None) == -1
  for bad in (0.0, 1.0, -1.0, float('nan')):
    assert lib.ms_relocate_fresh(64, 64, 3, 64, 10, bad, 64, 64, 64, 64, None) == -1
    assert b'min_opacity' in lib.ms_last_error_string()
  assert lib.ms_relocate_fresh(64, 64, 3, 64, 10, 0.005, None, 64, 64, 64, None) == -1
  assert lib.ms_relocate_fresh(None, None, 3, None, 0, 0.005, None, None, None, None, None) == 0

  assert lib.ms_perturb_positions(64, 64, 64, 64, 64, -1, 0.1, 100.0, 0.995, None) == -1
  assert lib.ms_perturb_positions(64, 64, 64, 64, 64, 1 << 31, 0.1, 100.0, 0.995, None) == -1
  assert lib.ms_perturb_positions(64, 64, None, 64, 64, 10, 0.1, 100.0, 0.995, None) == -1
  assert lib.ms_perturb_positions(64, 66, 64, 64, 64, 10, 0.1, 100.0, 0.995, None) == -1
  assert lib.ms_perturb_positions(64, 64, 64, 64, 64, 10, float('nan'), 100.0, 0.995, None) == -1
  assert lib.ms_perturb_positions(64, 64, 64, 64, 64, 10, 0.1, float('nan'), 0.995, None) == -1
  assert lib.ms_perturb_positions(None, None, None, None, None, 0, 0.1, 100.0, 0.995, None) == 0
