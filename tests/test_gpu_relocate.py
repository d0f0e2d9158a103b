"""Fixed-budget densification on the GPU (csrc/relocate.hip) against tests/relocate_oracle.py: weights, draw, corrected
opacity and scale, the in-place move of every role and row length, the position noise, graph capture, and one
ParameterClass end to end."""
import numpy as np
import pytest
import torch

from taichi_splatting_amd import _lib
from tests import relocate_oracle as oracle

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SIZES = [1, 2, 63, 64, 65, 257, 4097]       # one lane, a wave edge, a block edge, several blocks
POPULATIONS = ['no_dead', 'all_dead', 'one_live', 'random30']
MIN_OPACITY = 0.005
COPY, ZERO, INHERIT, OPACITY, SCALE = (_lib.RELOCATE_COPY, _lib.RELOCATE_ZERO_TOUCHED, _lib.RELOCATE_INHERIT,
                                       _lib.RELOCATE_OPACITY, _lib.RELOCATE_SCALE)
# name: (row shape, role).  Row lengths 4, 12, 16 and 192 bytes; `offset16` has 16-byte rows on a base 4 bytes off a
# 16-byte boundary, so it moves as 4-byte pieces while `rotation` moves as 16-byte pieces.
ARRAYS = {
  'position': ((3,), COPY), 'label': ((), COPY), 'rotation': ((4,), COPY), 'feature': ((3, 16), COPY),
  'offset16': ((4,), COPY), 'moment1': ((3,), ZERO), 'moment2': ((), ZERO), 'wide_moment': ((3, 16), ZERO),
  'running_vis': ((), INHERIT), 'alpha_logit': ((1,), OPACITY), 'log_scaling': ((3,), SCALE),
}


def bits(t):
  return t.detach().cpu().contiguous().view(torch.int32)


def scene(n, population, seed=0):
  """CPU float32 tensors of ARRAYS, (N,) int64 random words, and the dead mask."""
  g = torch.Generator().manual_seed(1000 * seed + n)
  host = {name: torch.randn((n, *shape), generator=g) for name, (shape, _) in ARRAYS.items()}
  alpha = (2.0 * torch.randn(n, generator=g)).clamp(-4.0, 12.0)           # live: above logit(0.005) = -5.29
  if population == 'all_dead':
    dead = torch.ones(n, dtype=torch.bool)
  elif population == 'one_live':
    dead = torch.ones(n, dtype=torch.bool)
    dead[n // 2] = False
  elif population == 'random30':
    dead = torch.rand(n, generator=g) < 0.3
  else:
    dead = torch.zeros(n, dtype=torch.bool)
  low = torch.where(torch.rand(n, generator=g) < 0.5, torch.full((n,), -10.0), -5.3 - torch.rand(n, generator=g))
  low[::7] = float('nan')                                                  # NaN is dead
  low[3::7] = float(oracle.threshold(MIN_OPACITY))                         # exactly the threshold: dead
  alpha = torch.where(dead, low, alpha)
  if population == 'random30' and n >= 63:
    live = (~dead).nonzero().squeeze(1)
    alpha[live[0]] = 17.0                                                  # o = 1 - 4e-8: the clamp at 1 - 1e-7
    alpha[live[1]] = float(np.nextafter(oracle.threshold(MIN_OPACITY), np.float32(0)))   # the faintest live row
  host['alpha_logit'] = alpha.reshape(n, 1)
  random = torch.randint(torch.iinfo(torch.int64).min, torch.iinfo(torch.int64).max, (n,), generator=g)
  return host, random, dead


def upload(host):
  """Device tensors; `offset16` is placed 4 bytes off a 16-byte boundary."""
  out = {}
  for name, t in host.items():
    if name == 'offset16':
      store = torch.zeros(t.numel() + 1, device=DEV)
      out[name] = store[1:].view(t.shape)
      out[name].copy_(t)
      assert out[name].data_ptr() % 16 == 4
    else:
      out[name] = t.to(DEV).contiguous()
      assert out[name].data_ptr() % 16 == 0
  return out


def run(host, random):
  from taichi_splatting_amd.optim.relocate import relocate_arrays
  dev = upload(host)
  result = relocate_arrays(dev['alpha_logit'], dev['log_scaling'], [(dev[name], role) for name, (_, role) in ARRAYS.items()],
                           min_opacity=MIN_OPACITY, random=random.to(DEV))
  torch.cuda.synchronize()
  return dev, result


def within_ulps(got32, want64, ulps):
  want64 = np.asarray(want64, dtype=np.float64)
  return np.abs(got32.astype(np.float64) - want64) <= ulps * np.spacing(np.abs(want64.astype(np.float32))).astype(np.float64)


@pytest.mark.parametrize('population', POPULATIONS)
@pytest.mark.parametrize('n', SIZES)
def test_relocate_against_the_oracle(n, population):
  host, random, dead = scene(n, population)
  dev, result = run(host, random)
  words = random.numpy().astype(np.uint64)
  alpha = host['alpha_logit'].numpy()

  # weights: dead rows exactly (a float32 comparison), live rows within one unit (device exp against numpy's)
  weights = result.weights.cpu().numpy()
  want_w = oracle.weights(alpha, MIN_OPACITY)
  assert np.array_equal(weights == 0, dead.numpy()) and np.array_equal(want_w == 0, dead.numpy())
  assert np.abs(weights - want_w).max() <= 1 and weights[~dead.numpy()].min(initial=1) >= 1

  # with the kernel's own weights the draw is exact
  src, count, total = oracle.draw(weights, words)
  got_src, got_count = result.src.cpu().numpy(), result.count.cpu().numpy()
  assert np.array_equal(got_src, src) and np.array_equal(got_count, count)
  moved, drawn = src != np.arange(n), count > 0
  assert result.counts.cpu().tolist() == [int(dead.sum()), int(drawn.sum()), total]
  assert not (drawn & dead.numpy()).any() and np.array_equal(moved, dead.numpy() & (total > 0))
  touched = moved | drawn
  mixed = bool(dead.any()) and not bool(dead.all())
  assert bool(moved.any()) == bool(drawn.any()) == bool(touched.any()) == mixed
  if population != 'random30':
    assert mixed == (population == 'one_live' and n >= 2)
  if population == 'random30' and n >= 63:
    assert mixed
  if population == 'one_live' and n >= 65:
    assert count.max() + 1 > oracle.MAX_RATIO                   # the ratio clamps at 51
  if population == 'one_live' and n >= 2:
    # the in-place hazard: a source in the same 16-byte piece as a dead row that copies it (4- and 12-byte rows)
    for row_bytes in (4, 12):
      pieces = lambda r: set(range((r * row_bytes) // 16, (r * row_bytes + row_bytes - 1) // 16 + 1))
      assert any(pieces(i) & pieces(src[i]) for i in np.nonzero(moved)[0])

  # opacity and scale of the touched rows: float64 oracle, rounded once, within 2 float32 ulp
  want_a, want_ls = oracle.fresh(alpha, host['log_scaling'].numpy(), count, MIN_OPACITY)
  got_a, got_ls = dev['alpha_logit'].cpu().numpy().reshape(-1), dev['log_scaling'].cpu().numpy()
  if touched.any():
    rows = np.nonzero(touched)[0]
    ulps_a = np.abs(got_a[rows] - want_a[src[rows]]) / np.spacing(np.abs(want_a[src[rows]].astype(np.float32)))
    ulps_s = np.abs(got_ls[rows] - want_ls[src[rows]]) / np.spacing(np.abs(want_ls[src[rows]].astype(np.float32)))
    print(f"n={n} {population}: opacity off by at most {ulps_a.max():.3f} ulp, scale by {ulps_s.max():.3f} ulp")
    assert within_ulps(got_a[rows], want_a[src[rows]], 2).all()
    assert within_ulps(got_ls[rows], want_ls[src[rows]], 2).all()
    assert np.isfinite(got_a[rows]).all() and np.isfinite(got_ls[rows]).all()
    # a copy and its source carry the same bits
    assert np.array_equal(got_a[rows].view(np.int32), got_a[src[rows]].view(np.int32))
    assert np.array_equal(got_ls[rows].view(np.int32), got_ls[src[rows]].view(np.int32))

  t_src, t_moved, t_touched = torch.from_numpy(src), torch.from_numpy(moved), torch.from_numpy(touched)
  for name, (_, role) in ARRAYS.items():
    before, after = bits(host[name]).reshape(n, -1), bits(dev[name]).reshape(n, -1)
    # untouched rows are bitwise unchanged in every array
    assert torch.equal(after[~t_touched], before[~t_touched]), name
    if role in (COPY, INHERIT):
      assert torch.equal(after[t_moved], before[t_src[t_moved]]), name        # a dead row is its source's row, bit for bit
      assert torch.equal(after[~t_moved], before[~t_moved]), name              # a drawn live row keeps its own
    elif role == ZERO:
      assert not after[t_touched].any(), name


@pytest.mark.parametrize('n', [65, 4097])
def test_two_runs_with_the_same_words_give_identical_bits(n):
  host, random, _ = scene(n, 'random30', seed=3)
  first, r1 = run(host, random)
  second, r2 = run(host, random)
  for name in ARRAYS:
    assert torch.equal(bits(first[name]), bits(second[name])), name
  for field in ('src', 'count', 'weights', 'counts'):
    assert torch.equal(getattr(r1, field), getattr(r2, field)), field
  other, r3 = run(host, torch.roll(random, 1))
  assert not torch.equal(r1.src, r3.src)


@pytest.mark.parametrize('population', ['few_touched', 'many_touched'])
def test_rows_wider_than_a_block(population):
  """Rows of 255 .. 1024 pieces (tests/wide_rows.py) in every plain role, through both walks of the move: a block with
  at most one touched row in 8 walks its touched rows alone (RELOC_COMPACT_BELOW of csrc/relocate.hip), any other block
  all its rows.  Expected rows by torch indexing on copies of the inputs, compared on the bits."""
  from taichi_splatting_amd.optim.relocate import relocate_arrays
  from tests.wide_rows import N, bits, wide_arrays
  g = torch.Generator().manual_seed(11)
  alpha = (2.0 * torch.randn(N, generator=g)).clamp(-4.0, 12.0)
  dead = torch.zeros(N, dtype=torch.bool)
  if population == 'few_touched':
    dead[[3, 100, 200, 270]] = True           # with their sources at most 8 touched rows of 256 and 5 of 44
  else:
    dead[::3] = True                          # a third of every block, before any source
  alpha[dead] = -10.0
  random = torch.randint(torch.iinfo(torch.int64).min, torch.iinfo(torch.int64).max, (N,), generator=g)
  log_scaling = torch.randn(N, 3, generator=g)

  roles = (COPY, ZERO, INHERIT)
  arrays = {(name, role): t for role in roles for name, t in wide_arrays(DEV).items()}
  before = {key: t.clone() for key, t in arrays.items()}
  result = relocate_arrays(alpha.reshape(N, 1).to(DEV), log_scaling.to(DEV), [(t, role) for (_, role), t in arrays.items()],
                           min_opacity=MIN_OPACITY, random=random.to(DEV))
  torch.cuda.synchronize()

  src, count, _ = oracle.draw(result.weights.cpu().numpy(), random.numpy().astype(np.uint64))
  assert np.array_equal(result.src.cpu().numpy(), src) and np.array_equal(result.count.cpu().numpy(), count)
  moved, touched = src != np.arange(N), (src != np.arange(N)) | (count > 0)
  assert np.array_equal(moved, dead.numpy())
  per_block = [(int(touched[b:b + 256].sum()), len(touched[b:b + 256])) for b in range(0, N, 256)]
  assert [rows for _, rows in per_block] == [256, 44]
  print(f"{population}: touched rows per block {per_block}")
  if population == 'few_touched':
    assert all(0 < t and t * 8 <= rows for t, rows in per_block), per_block          # the compact walk, in both blocks
  else:
    assert all(t * 8 > rows for t, rows in per_block), per_block                      # the full walk, in both blocks

  t_src, t_moved, t_touched = (torch.from_numpy(x).to(DEV) for x in (src.astype(np.int64), moved, touched))
  for (name, role), t in arrays.items():
    want = before[(name, role)].clone()
    if role == ZERO:
      want[t_touched] = 0.0
    else:
      want[t_moved] = before[(name, role)][t_src[t_moved]]
    assert torch.equal(bits(t), bits(want)), (name, role)


# ---- position noise ---------------------------------------------------------------------------------------------------

def noise_scene(n, seed=0):
  g = torch.Generator().manual_seed(77 * seed + n)
  rand = lambda *shape: torch.randn(*shape, generator=g)
  host = dict(position=3.0 * rand(n, 3), log_scaling=0.7 * rand(n, 3) - 1.0,
              rotation=rand(n, 4) * (0.25 + 2.0 * torch.rand(n, 1, generator=g)),       # not normalised
              alpha_logit=torch.where(torch.rand(n, 1, generator=g) < 0.5, -6.0 + rand(n, 1), 3.0 * rand(n, 1)))
  z = rand(n, 3)
  z[1::5] = 0.0
  return host, z


def perturbed(host, z, step, k, x0, zero_position=False):
  from taichi_splatting_amd import Gaussians3D, perturb_positions
  n = z.shape[0]
  g = Gaussians3D(position=torch.zeros_like(host['position']) if zero_position else host['position'].clone(),
                  log_scaling=host['log_scaling'], rotation=host['rotation'], alpha_logit=host['alpha_logit'],
                  feature=torch.zeros(n, 3), batch_size=[n]).to(DEV)
  assert perturb_positions(g, step, z=z.to(DEV), k=k, x0=x0) is g
  torch.cuda.synchronize()
  return g.position.cpu()


@pytest.mark.parametrize('k', [100.0, 1e5])
@pytest.mark.parametrize('n', SIZES)
def test_perturb_positions_against_the_oracle(n, k):
  """From a zero position the new position IS the kernel's offset d, which is held to the bound
  |d - d_oracle| <= 1e-5 step g |Sigma|_max |z|_1; from the real positions the result is float32(p + d) of that offset,
  bit for bit.  k = 1e5 makes g exactly 0 for the visible gaussians and 1 for the faintest.
  d is a float32.  At k = 100 an opaque gaussian has g = e^-99.5 = 6e-44 and an offset far below the float32 normal
  range, where the spacing of float32 is 2^-149 whatever the value: a row whose bound is finer than that spacing is held
  to the spacing (no float32 can do better than half of it), every other row to the bound as it stands."""
  host, z = noise_scene(n)
  step, x0 = 0.37, 0.995
  want, g, sigma_max = oracle.perturbation(host['log_scaling'].numpy(), host['rotation'].numpy(), host['alpha_logit'].numpy(),
                                           z.numpy(), np.float32(step).astype(np.float64), k, x0)
  bound = 1e-5 * step * g * sigma_max * np.abs(z.numpy().astype(np.float64)).sum(1)
  held = np.maximum(bound, 2.0 ** -149)
  offset = perturbed(host, z, step, k, x0, zero_position=True)
  err = np.abs(offset.numpy().astype(np.float64) - want).max(1)
  normal = bound >= 2.0 ** -149
  ratio = float((err[normal] / bound[normal]).max()) if normal.any() else 0.0
  print(f"perturb n={n} k={k:g}: largest |d - d_oracle| / bound = {ratio:.4f} over {int(normal.sum())} rows "
        f"({int((~normal).sum())} rows with a bound under 2^-149: largest error {err[~normal].max(initial=0.0):.3g})")
  assert (err <= held).all()

  moved = perturbed(host, z, step, k, x0)
  assert torch.equal(bits(moved), bits(host['position'] + offset))
  still = torch.from_numpy((g == 0) | (np.abs(z.numpy()).sum(1) == 0))
  assert torch.equal(bits(moved)[still], bits(host['position'])[still])          # g = 0 or z = 0: bitwise unchanged
  if n >= 63:
    assert still.any() and not still.all()
    if k == 1e5:
      assert (g == 0).any() and (g == 1).any()

  # the unnormalised quaternion against its normalised form, to the same bound
  q = host['rotation'].double()
  unit = dict(host, rotation=(q / q.norm(dim=1, keepdim=True)).float())
  offset_unit = perturbed(unit, z, step, k, x0, zero_position=True)
  assert (np.abs((offset_unit - offset).numpy().astype(np.float64)).max(1) <= held).all()


def test_perturb_positions_on_a_misaligned_scene_and_a_zero_quaternion():
  """The 4-byte path (a position 4 bytes off a 16-byte boundary) gives the bits of the 16-byte path; a zero quaternion
  has no covariance and the row stays."""
  from taichi_splatting_amd import Gaussians3D, perturb_positions
  n = 321
  host, z = noise_scene(n, seed=2)
  host['rotation'][5] = 0.0
  aligned = perturbed(host, z, 0.2, 100.0, 0.995)
  store = torch.zeros(3 * n + 1, device=DEV)
  position = store[1:].view(n, 3)
  position.copy_(host['position'])
  assert position.data_ptr() % 16 == 4
  g = Gaussians3D(position=position, log_scaling=host['log_scaling'].to(DEV), rotation=host['rotation'].to(DEV),
                  alpha_logit=host['alpha_logit'].to(DEV), feature=torch.zeros(n, 3, device=DEV), batch_size=[n])
  perturb_positions(g, 0.2, z=z.to(DEV))
  assert torch.equal(bits(position), bits(aligned)) and float(store[0]) == 0.0
  assert torch.equal(bits(aligned)[5], bits(host['position'])[5])
  assert not torch.equal(bits(aligned), bits(host['position'])) and bool(torch.isfinite(aligned).all())


# ---- capture: no host read ---------------------------------------------------------------------------------------------

def test_relocate_and_perturb_replay_from_a_graph():
  from taichi_splatting_amd import Gaussians3D, perturb_positions
  from taichi_splatting_amd.optim.relocate import relocate_arrays
  n = 4097
  host, random, _ = scene(n, 'random30', seed=5)

  def step(dev, words, z):
    result = relocate_arrays(dev['alpha_logit'], dev['log_scaling'], [(dev[name], role) for name, (_, role) in ARRAYS.items()],
                             min_opacity=MIN_OPACITY, random=words)
    g = Gaussians3D(position=dev['position'], log_scaling=dev['log_scaling'], rotation=dev['rotation'],
                    alpha_logit=dev['alpha_logit'], feature=dev['feature'], batch_size=[n])
    perturb_positions(g, 0.05, z=z)
    return result

  gen = torch.Generator().manual_seed(11)
  draws = [(torch.randint(torch.iinfo(torch.int64).min, torch.iinfo(torch.int64).max, (n,), generator=gen),
            torch.randn(n, 3, generator=gen)) for _ in range(2)]
  eager = []
  for words, z in draws:                 # also the warm-up every capture needs
    dev = upload(host)
    eager.append((dev, step(dev, words.to(DEV), z.to(DEV))))
  torch.cuda.synchronize()

  static = upload(host)
  words, z = random.to(DEV), torch.zeros(n, 3, device=DEV)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    captured = step(static, words, z)
  for (new_words, new_z), (want, want_result) in zip(draws, eager):
    for name, t in host.items():
      static[name].copy_(t)
    words.copy_(new_words)
    z.copy_(new_z)
    graph.replay()
    torch.cuda.synchronize()
    for name in ARRAYS:
      assert torch.equal(bits(static[name]), bits(want[name])), name
    for field in ('src', 'count', 'weights', 'counts'):
      assert torch.equal(getattr(captured, field), getattr(want_result, field)), field
  assert not torch.equal(eager[0][1].src, eager[1][1].src)


# ---- ParameterClass ---------------------------------------------------------------------------------------------------

FIELDS3D = ('position', 'log_scaling', 'rotation', 'alpha_logit', 'feature')


def trained_params(n, seed=0):
  """A ParameterClass over a small Gaussians3D after three VisibilityAwareAdam steps: every state tensor is non-zero."""
  from taichi_splatting_amd import Gaussians3D
  from taichi_splatting_amd.optim import ParameterClass, VisibilityAwareAdam
  g = torch.Generator(device=DEV).manual_seed(seed)
  rand = lambda *shape: torch.randn(*shape, device=DEV, generator=g)
  points = Gaussians3D(position=rand(n, 3), log_scaling=rand(n, 3), rotation=rand(n, 4), alpha_logit=rand(n, 1),
                       feature=rand(n, 3, 16), batch_size=[n])
  params = ParameterClass({k: getattr(points, k) for k in FIELDS3D}, {k: dict(lr=0.01) for k in FIELDS3D},
                          optimizer=VisibilityAwareAdam)

  def step():
    for k in FIELDS3D:
      params.tensors[k].grad = rand(*params.tensors[k].shape)
    params.step(indexes=torch.arange(n, device=DEV), visibility=torch.rand(n, device=DEV, generator=g) + 0.1)

  for _ in range(3):
    step()
  return params, step


def test_parameter_class_end_to_end():
  n = 257
  params, step = trained_params(n)
  with torch.no_grad():
    params.tensors['alpha_logit'][::3] = -10.0
  addresses = {k: t.data_ptr() for k, t in params.tensors.items()}
  state_before = {(k, s): t.clone() for k, st in params.tensor_state.items() for s, t in st.items()}
  state_addresses = {key: t.data_ptr() for key, t in ((key, params.tensor_state[key[0]][key[1]]) for key in state_before)}
  assert any(s == 'running_vis' for _, s in state_before), sorted(state_before)
  optimizer, before = params.optimizer, {k: t.detach().clone() for k, t in params.tensors.items()}

  result = params.relocate(min_opacity=MIN_OPACITY, inherit_state=('running_vis',))
  src = result.src.long()
  moved, touched = src != torch.arange(n, device=DEV), (src != torch.arange(n, device=DEV)) | (result.count > 0)
  assert result.counts.tolist()[:1] == [len(range(0, n, 3))] and int(moved.sum()) == len(range(0, n, 3))
  assert params.optimizer is optimizer
  for k, t in params.tensors.items():
    assert t.data_ptr() == addresses[k] and t.requires_grad, k
    if k not in ('alpha_logit', 'log_scaling'):
      assert torch.equal(t.detach(), before[k][src]), k
    assert torch.equal(t.detach()[~touched], before[k][~touched]), k
  for (k, s), old in state_before.items():
    new = params.tensor_state[k][s]
    assert new.data_ptr() == state_addresses[(k, s)], (k, s)
    assert torch.equal(new[~touched], old[~touched]), (k, s)
    if s == 'running_vis':                       # inherit_state is honoured: the state follows the gaussian
      assert torch.equal(new, old[src]), (k, s)
    else:
      assert not new[touched].any() and bool(old[touched].any()), (k, s)

  after_relocate = {k: t.detach().clone() for k, t in params.tensors.items()}
  step()                                         # the optimiser still steps, on the same storage
  for k, t in params.tensors.items():
    assert t.data_ptr() == addresses[k] and not torch.equal(t.detach(), after_relocate[k]), k
    assert bool(torch.isfinite(t).all()), k


def test_gaussians3d_form_and_a_state_that_is_not_per_point():
  from taichi_splatting_amd import Gaussians3D, relocate_gaussians3d
  from taichi_splatting_amd.optim import ParameterClass
  n = 257
  host, random, dead = scene(n, 'random30', seed=7)
  fields = {k: host[k].to(DEV) for k in FIELDS3D}
  points = Gaussians3D(**{k: v.clone() for k, v in fields.items()}, batch_size=[n])
  result = relocate_gaussians3d(points, min_opacity=MIN_OPACITY, random=random.to(DEV))
  dev, want = run(host, random)
  assert torch.equal(result.src, want.src) and torch.equal(result.count, want.count)
  for k in FIELDS3D:
    assert torch.equal(bits(getattr(points, k)), bits(dev[k])), k

  # the default words come from torch's generator: reproducible under a seed
  outcomes = []
  for _ in range(2):
    torch.manual_seed(3)
    again = Gaussians3D(**{k: v.clone() for k, v in fields.items()}, batch_size=[n])
    outcomes.append(relocate_gaussians3d(again, min_opacity=MIN_OPACITY).src)
  assert torch.equal(outcomes[0], outcomes[1]) and not torch.equal(outcomes[0], result.src)

  # torch's Adam keeps a 0-d `step` tensor in its state: not per point, refused as densify refuses it
  params = ParameterClass(fields, {k: dict(lr=0.01) for k in FIELDS3D}, optimizer=torch.optim.Adam)
  for k in FIELDS3D:
    params.tensors[k].grad = torch.ones_like(params.tensors[k])
  params.step()
  with pytest.raises(AssertionError, match="not per point"):
    params.relocate()
