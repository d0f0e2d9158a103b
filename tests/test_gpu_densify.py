"""-m gpu: fused densification (csrc/densify.hip, optim/densify.py, misc/densify.py) against the torch path —
``params[keep].append_tensors(children)`` and the split helpers of misc/renderer2d.py — never against itself.

Moved rows are copies: every comparison of moved rows is ``torch.equal``.  Child geometry: the torch functions are
evaluated in float64 and in float32 on the same inputs, ``d32`` is the largest float32-vs-float64 deviation of a field,
and the kernel has to stay within ``4 * d32`` of the float64 result (same operations; other exp / rsqrt implementations
and contraction).  Both figures are printed (``pytest -s``)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def optimisers():
  from taichi_splatting_amd import optim
  return dict(FractionalAdam=optim.FractionalAdam, FractionalLaProp=optim.FractionalLaProp, SparseAdam=optim.SparseAdam,
              SparseLaProp=optim.SparseLaProp, VisibilityAwareAdam=optim.VisibilityAwareAdam,
              VisibilityAwareLaProp=optim.VisibilityAwareLaProp)


def stepped_params(n, optimiser='VisibilityAwareAdam', tensors=None, groups=None, seed=0):
  """A ParameterClass with the five Gaussians3D fields after three real step() calls: every state tensor exists and is
  non-zero (moments of both shapes, total_weight, running_vis)."""
  from taichi_splatting_amd.optim import ParameterClass
  g = torch.Generator(device=DEV).manual_seed(seed + n)
  rand = lambda *shape: torch.randn(*shape, device=DEV, generator=g)
  if tensors is None:
    tensors = dict(position=rand(n, 3), log_scaling=rand(n, 3), rotation=rand(n, 4), alpha_logit=rand(n, 1),
                   feature=rand(n, 3, 16))
    groups = dict(position=dict(lr=0.1, type='vector'), log_scaling=dict(lr=0.05), rotation=dict(lr=0.05),
                  alpha_logit=dict(lr=0.1), feature=dict(lr=0.02, type='vector'))
  params = ParameterClass(tensors, groups, optimizer=optimisers()[optimiser])
  indexes = torch.arange(n, device=DEV)
  for _ in range(3):
    for k in groups:
      params.tensors[k].grad = torch.randn(params.tensors[k].shape, device=DEV, generator=g)
    weight = torch.rand(n, device=DEV, generator=g) + 0.1
    if optimiser.startswith('Sparse'):
      params.step(indexes=indexes)
    elif optimiser.startswith('Fractional'):
      params.step(indexes=indexes, weight=weight)
    else:
      params.step(indexes=indexes, visibility=weight)
  for name, st in params.tensor_state.items():
    for key, t in st.items():
      assert t.shape[0] == n and bool((t != 0).any()), (name, key)
  return params


def masks(case, n, seed=0):
  g = torch.Generator(device=DEV).manual_seed(seed * 7919 + n)
  flags = lambda p: torch.rand(n, device=DEV, generator=g) < p
  none = torch.zeros(n, dtype=torch.bool, device=DEV)
  if case == 'identity':
    return none, none.clone()
  if case == 'prunes':
    prune = flags(0.3)
    prune[0] = True
    return prune, none
  if case == 'splits':
    split = flags(0.3)
    split[-1] = True
    return none, split
  if case == 'all_split':
    return none, ~none
  if case == 'both_same':            # the same rows carry both flags: pruned
    both = flags(0.4)
    both[0] = True
    return both, both.clone()
  assert case == 'mixed'             # independent flags, overlapping on some rows
  return flags(0.3), flags(0.4)


CASES = ('identity', 'prunes', 'splits', 'all_split', 'both_same', 'mixed')


def torch_path(params, prune, split, n_children):
  """What the parent commit computes: params[keep].append_tensors(children) with torch-made children (parent copies);
  returns (tensors, tensor_state, ParameterClass or None when params[keep] would be empty)."""
  split_only = split & ~prune
  keep = ~(prune | split)
  children = {k: torch.repeat_interleave(t.detach()[split_only], n_children, dim=0) for k, t in params.tensors.items()}
  if bool(keep.any()):
    ref = params[keep].append_tensors(children)
    return {k: t.detach() for k, t in ref.tensors.items()}, ref.tensor_state, ref
  tensors = {k: torch.cat([t.detach()[keep], children[k]]) for k, t in params.tensors.items()}
  state = {name: {key: torch.cat([t[keep], t.new_zeros((children[name].shape[0], *t.shape[1:]))]) for key, t in st.items()}
           for name, st in params.tensor_state.items()}
  return tensors, state, None


def assert_same(out, params, prune, split, n_children):
  tensors, state, ref = torch_path(params, prune, split, n_children)
  assert list(out.keys()) == list(params.keys())
  for k, want in tensors.items():
    got = out.tensors[k].detach()
    assert got.shape == want.shape and got.dtype == want.dtype, (k, got.shape, want.shape)
    assert torch.equal(got, want), k
    assert isinstance(out.tensors[k], torch.nn.Parameter) == isinstance(params.tensors[k], torch.nn.Parameter), k
  got_state = out.tensor_state
  assert {k: set(v) for k, v in got_state.items()} == {k: set(v) for k, v in state.items()}
  n_kept = int((~(prune | split)).sum())
  for name, st in state.items():
    for key, want in st.items():
      got = got_state[name][key]
      assert got.shape == want.shape and torch.equal(got, want), (name, key)
      assert not bool(got[n_kept:].any()), (name, key, "child state must be zero")
  assert out.parameter_groups == params.parameter_groups
  assert out.other_state == params.other_state
  assert type(out.optimizer) is type(params.optimizer) and out.optim_kwargs == params.optim_kwargs
  if ref is not None:
    assert out.parameter_groups == ref.parameter_groups and out.other_state == ref.other_state
    assert list(out.keys()) == list(ref.keys())


@pytest.mark.parametrize('n', [1, 255, 256, 257, 100003])
def test_moved_rows_equal_the_torch_path(n):
  params = stepped_params(n)
  for case in CASES:
    prune, split = masks(case, n)
    if int((~prune).sum()) == 0:               # nothing left: refused, as ParameterClass refuses an empty collection
      with pytest.raises(ValueError, match="no rows left"):
        params.densify(prune, split, 2)
      with pytest.raises(AssertionError):
        params[~(prune | split)]
      continue
    assert_same(params.densify(prune, split, 2), params, prune, split, 2)
  # uint8 masks are taken as they are
  prune, split = masks('mixed', n, seed=1)
  if int((~prune).sum()) > 0:
    assert_same(params.densify(prune.to(torch.uint8), split.to(torch.uint8) * 3, 2), params, prune, split, 2)


@pytest.mark.parametrize('optimiser', sorted(optimisers()))
def test_every_optimiser_keeps_its_state(optimiser):
  n = 1000
  params = stepped_params(n, optimiser)
  for children in (1, 2, 3):
    prune, split = masks('mixed', n, seed=children)
    assert_same(params.densify(prune, split, children), params, prune, split, children)
  if optimiser.startswith('Visibility'):       # optionally the running visibility is inherited
    prune, split = masks('mixed', n, seed=5)
    out = params.densify(prune, split, 2, inherit_state=('running_vis',))
    n_kept = int((~(prune | split)).sum())
    parents = (split & ~prune).nonzero().squeeze(1).repeat_interleave(2)
    first = next(iter(params.optimized_keys()))
    assert torch.equal(out.tensor_state[first]['running_vis'][n_kept:], params.tensor_state[first]['running_vis'][parents])
    assert not bool(out.tensor_state[first]['total_weight'][n_kept:].any())


def test_row_widths_of_every_residue_and_an_unaligned_source():
  from taichi_splatting_amd.optim.densify import move_rows, plan_densify
  n = 4099
  g = torch.Generator(device=DEV).manual_seed(3)
  widths = (1, 2, 3, 4, 7, 48)
  tensors = {f'w{w}': torch.randn(n, w, device=DEV, generator=g) for w in widths}
  tensors['fixed'] = torch.randn(n, 5, device=DEV, generator=g)           # not optimised: moved too
  groups = {f'w{w}': dict(lr=0.01) for w in widths}
  params = stepped_params(n, 'SparseAdam', tensors, groups)
  for children in (1, 2, 3):
    prune, split = masks('mixed', n, seed=children)
    assert_same(params.densify(prune, split, children), params, prune, split, children)

  # a source whose base is 4 bytes into an allocation: rows of 16 and 192 bytes must take the 4-byte pieces
  prune, split = masks('mixed', n, seed=9)
  plan = plan_densify(prune, split, 2)
  keep, split_only = ~(prune | split), split & ~prune
  assert (plan.n_kept, plan.n_split, plan.n_out) == (int(keep.sum()), int(split_only.sum()), int(keep.sum()) + 2 * int(split_only.sum()))
  assert plan.counts.tolist() == [plan.n_kept, plan.n_split, plan.n_out, n]
  assert torch.equal(plan.parent_rows, split_only.nonzero().squeeze(1))
  for w in (4, 48):
    buffer = torch.randn(n * w + 1, device=DEV, generator=g)
    src = buffer[1:].view(n, w)
    assert src.data_ptr() % 16 == 4 and src.is_contiguous()
    copied, zeroed = move_rows(plan, [(src, True), (src, False)])
    children = src[split_only].repeat_interleave(2, dim=0)
    assert torch.equal(copied, torch.cat([src[keep], children]))
    assert torch.equal(zeroed, torch.cat([src[keep], torch.zeros_like(children)]))


@pytest.mark.parametrize('children', [1, 3])
def test_rows_wider_than_a_block(children):
  """Rows of 255 .. 1024 pieces (tests/wide_rows.py): a lane's walk starts in row 0 and carries at most once per step.
  Expected rows by torch indexing on copies of the inputs, compared on the bits."""
  from taichi_splatting_amd.optim.densify import move_rows, plan_densify
  from tests.wide_rows import N, bits, wide_arrays
  arrays = wide_arrays(DEV)
  before = {name: t.clone() for name, t in arrays.items()}
  prune, split = masks('mixed', N, seed=children)
  keep, split_only = ~(prune | split), split & ~prune
  plan = plan_densify(prune, split, children)
  assert plan.n_out == int(keep.sum()) + children * int(split_only.sum()) and plan.n_split > 0 and plan.n_kept > 0
  moved = move_rows(plan, [(t, fill) for t in arrays.values() for fill in (True, False)])
  torch.cuda.synchronize()
  for i, (name, t) in enumerate(arrays.items()):
    assert torch.equal(bits(t), bits(before[name])), name                     # the sources are read only
    parents = before[name][split_only].repeat_interleave(children, dim=0)
    copied, zeroed = moved[2 * i], moved[2 * i + 1]
    assert copied.shape == zeroed.shape == (plan.n_out, t.shape[1]), name
    assert torch.equal(bits(copied), bits(torch.cat([before[name][keep], parents]))), name
    assert torch.equal(bits(zeroed), bits(torch.cat([before[name][keep], torch.zeros_like(parents)]))), name


def deviations(fields, kernel, f32, f64, label):
  """Asserts |kernel - f64| <= 4 d32 with d32 = max |f32 - f64| per field; prints both."""
  for k in fields:
    d32 = float((f32[k].double() - f64[k]).abs().max())
    dk = float((kernel[k].double() - f64[k]).abs().max())
    print(f"{label} {k}: d32 = {d32:.3e}, kernel = {dk:.3e}")
    assert dk <= 4 * d32, (label, k, dk, d32)


def split2d_reference(parents, z, factor, n, dtype):
  """The children of misc/renderer2d.py: ``factor`` a number (split_gaussians2d: both axes) or (P, 2) per-axis factors
  (uniform_split_gaussians2d: set_scaling)."""
  from taichi_splatting_amd.misc.renderer2d import repeat_sample_gaussians, split_with_offsets
  p = parents.to(dtype=dtype)
  offsets = repeat_sample_gaussians(z.to(dtype), p, n)
  if torch.is_tensor(factor):
    shrunk = p.set_scaling(p.scaling * factor.to(dtype))
  else:
    shrunk = p.replace(log_scaling=p.log_scaling + math.log(factor))
  return split_with_offsets(shrunk, offsets, depth_noise=0)


FIELDS2D = ('position', 'depths', 'log_scaling', 'rotation', 'alpha_logit', 'feature')


@pytest.mark.parametrize('mode', ['isotropic', 'one_axis'])
def test_2d_children_against_renderer2d(mode):
  from taichi_splatting_amd.misc.densify import split_children2d
  from taichi_splatting_amd.optim import ParameterClass, SparseAdam
  from taichi_splatting_amd.testing import random_2d_gaussians
  torch.manual_seed(11)
  count, n = 20000, 2
  points = random_2d_gaussians(count, (640, 480), alpha_range=(0.5, 1.0), scale_factor=0.5).to(DEV)
  params = ParameterClass({k: getattr(points, k) for k in FIELDS2D},
                          {k: dict(lr=0.01) for k in FIELDS2D if k != 'depths'}, optimizer=SparseAdam)
  prune, split = masks('mixed', count, seed=2)
  split_only = split & ~prune
  parents = points[split_only]
  num = int(split_only.sum())
  z = 0.5 * torch.randn((num, n, 2), device=DEV)
  if mode == 'isotropic':
    factor = kernel_scale = 1.0 / math.sqrt(n)
  else:
    onehot = torch.nn.functional.one_hot(torch.randint(0, 2, (num,), device=DEV), num_classes=2)
    factor = onehot.double() * (math.sqrt(n) / n) + (1 - onehot.double())
    kernel_scale = onehot.float() * (math.sqrt(n) / n) + (1 - onehot.float())
  f64 = split2d_reference(parents, z, factor, n, torch.float64)
  f32 = split2d_reference(parents, z, factor, n, torch.float32)

  out = params.densify(prune, split, n,
                       split_fn=lambda tensors, plan: split_children2d(tensors, plan.n_kept, n, z, kernel_scale))
  n_kept = int((~(prune | split)).sum())
  assert out.batch_size[0] == n_kept + n * num
  kernel = {k: out.tensors[k].detach()[n_kept:] for k in FIELDS2D}
  for k in FIELDS2D:                                  # kept rows: copies
    assert torch.equal(out.tensors[k].detach()[:n_kept], getattr(points, k)[~(prune | split)]), k
  for k in ('rotation', 'alpha_logit', 'feature'):
    assert torch.equal(kernel[k], getattr(f32, k)), k
  deviations(('position', 'log_scaling', 'depths'), kernel, {k: getattr(f32, k) for k in FIELDS2D},
             {k: getattr(f64, k) for k in FIELDS2D}, f"2-D {mode}")


def split3d_restatement(position, log_scaling, rotation, z, scale, dtype):
  """offset = R(q / |q|) (exp(log_scaling) * z), log_scaling += log(scale): children grouped by parent."""
  from oracle.projection import quat_to_mat
  position, log_scaling, rotation, z, scale = (t.to(dtype) for t in (position, log_scaling, rotation, z, scale))
  n = z.shape[1]
  R = quat_to_mat(rotation / torch.norm(rotation, dim=1, keepdim=True))
  offsets = torch.einsum('pij,pkj->pki', R, torch.exp(log_scaling).unsqueeze(1) * z)
  return dict(position=torch.repeat_interleave(position, n, dim=0) + offsets.reshape(-1, 3),
              log_scaling=torch.repeat_interleave(log_scaling + torch.log(scale), n, dim=0))


def scene3d(count, size=(160, 96)):
  from taichi_splatting_amd.testing import random_camera, random_3d_gaussians
  cam = random_camera(image_size=size)
  g = random_3d_gaussians(count, cam, scale_factor=1.0, alpha_range=(0.1, 0.9))
  g = g.replace(feature=(torch.rand(count, 3, 16) - 0.5) * 0.5, rotation=g.rotation * (0.5 + torch.rand(count, 1)))
  return g.to(DEV), cam.to(device=DEV)


FIELDS3D = ('position', 'log_scaling', 'rotation', 'alpha_logit', 'feature')


def params3d(points):
  from taichi_splatting_amd.optim import ParameterClass, VisibilityAwareAdam
  return ParameterClass({k: getattr(points, k) for k in FIELDS3D}, {k: dict(lr=0.01) for k in FIELDS3D},
                        optimizer=VisibilityAwareAdam)


@pytest.mark.parametrize('n', [2, 3])
def test_3d_children_against_a_float64_restatement(n):
  from taichi_splatting_amd.misc.densify import densify_split_gaussians3d, split_gaussians3d
  torch.manual_seed(5)
  count = 30000
  points, _ = scene3d(count)
  prune, split = masks('mixed', count, seed=4)
  split_only, keep = split & ~prune, ~(prune | split)
  num = int(split_only.sum())
  z = 0.5 * torch.randn((num, n, 3), device=DEV)
  scale = 0.5 + 0.5 * torch.rand((num, 3), device=DEV)
  parents = points[split_only]
  args = (parents.position, parents.log_scaling, parents.rotation, z, scale)
  f64, f32 = split3d_restatement(*args, torch.float64), split3d_restatement(*args, torch.float32)

  out = densify_split_gaussians3d(params3d(points), prune, split, n=n, scaling=scale, z=z)
  n_kept = int(keep.sum())
  assert out.batch_size[0] == n_kept + n * num
  for k in FIELDS3D:
    assert torch.equal(out.tensors[k].detach()[:n_kept], getattr(points, k)[keep]), k
  for k in ('rotation', 'alpha_logit', 'feature'):
    assert torch.equal(out.tensors[k].detach()[n_kept:], getattr(parents, k).repeat_interleave(n, dim=0)), k
  kernel = {k: out.tensors[k].detach()[n_kept:] for k in ('position', 'log_scaling')}
  deviations(('position', 'log_scaling'), kernel, f32, f64, f"3-D n={n}")

  # the direct form on Gaussians3D: the same kernel on repeat_interleave'd rows
  direct = split_gaussians3d(parents, n=n, scaling=scale, z=z)
  assert torch.equal(direct.position, kernel['position']) and torch.equal(direct.log_scaling, kernel['log_scaling'])
  assert torch.equal(direct.feature, parents.feature.repeat_interleave(n, dim=0))
  # the default draw (half a standard normal) and the default factor 1 / sqrt(n)
  torch.manual_seed(1)
  drawn = split_gaussians3d(parents, n=n)
  torch.manual_seed(1)
  z_drawn = 0.5 * torch.randn((num, n, 3), device=DEV)
  given = split_gaussians3d(parents, n=n, scaling=torch.full((num, 3), 1 / math.sqrt(n), device=DEV), z=z_drawn)
  assert torch.equal(drawn.position, given.position) and torch.equal(drawn.log_scaling, given.log_scaling)


def test_3d_children_with_zero_offsets_are_their_parents_and_render_the_same_image():
  from taichi_splatting_amd import RasterConfig, render_gaussians
  from taichi_splatting_amd.misc.densify import densify_split_gaussians3d, split_gaussians3d
  torch.manual_seed(0)
  count = 3000
  points, cam = scene3d(count)
  for n in (1, 2, 3):
    z = torch.zeros((count, n, 3), device=DEV)
    for scaling in (1.0, torch.ones((count, 3), device=DEV)):
      children = split_gaussians3d(points, n=n, scaling=scaling, z=z)
      for k in FIELDS3D:
        assert torch.equal(getattr(children, k), getattr(points, k).repeat_interleave(n, dim=0)), (k, n)

  # every row split into one child at its parent's place: a re-ordering that keeps storage order
  none = torch.zeros(count, dtype=torch.bool, device=DEV)
  out = densify_split_gaussians3d(params3d(points), none, ~none, n=1, scaling=1.0, z=torch.zeros((count, 1, 3), device=DEV))
  for k in FIELDS3D:
    assert torch.equal(out.tensors[k].detach(), getattr(points, k)), k
  from taichi_splatting_amd import Gaussians3D
  moved = Gaussians3D(**{k: out.tensors[k].detach() for k in FIELDS3D}, batch_size=(count,))
  cfg = RasterConfig()
  a = render_gaussians(points, cam, cfg, use_sh=True).image.detach()
  b = render_gaussians(moved, cam, cfg, use_sh=True).image.detach()
  assert torch.equal(a, b)


def test_fit_with_fused_densify_and_the_first_split_prune_in_both_modes():
  """End to end with the thresholds of tests/test_gpu_fit_image.py, then one split_prune of a seeded state in both modes:
  same masks, same draws, so the same rows; kept rows and state bit for bit, children within the bound of check 2."""
  from taichi_splatting_amd import Gaussians2D
  from taichi_splatting_amd.examples import fit_image_gaussians as demo
  ref = demo.test_card(192, 128, torch.device(DEV))
  image, params, history = demo.fit(ref, n=400, iters=240, target=800, seed=0, fused_densify=True)
  first, last = history[0][1], history[-1][1]
  assert all(torch.isfinite(t).all() for t in params.tensors.values())
  assert last > first + 4.0 and last > 19.0, history
  assert 700 <= params.batch_size[0] <= 800, params.batch_size
  assert image.shape == ref.shape and abs(demo.psnr(ref, image) - last) < 1e-3

  # the state after the first epoch of such a run (its last densification target included)
  _, params, _ = demo.fit(ref, n=400, iters=8, target=None, seed=0)
  config = demo.RasterConfig(compute_point_heuristic=True, compute_visibility=True, tile_size=16, blur_cov=0.3,
                             pixel_stride=(2, 2))
  _, heuristics = demo.train_epoch(params, ref, config, 2)
  results = []
  for fused in (False, True):
    torch.manual_seed(42)
    results.append(demo.split_prune(params, 0.1, 480, 0.025, heuristics, fused=fused))
  (want, want_counts), (got, got_counts) = results
  assert want_counts == got_counts and want_counts['split'] > 0 and want_counts['prune'] > 0, (want_counts, got_counts)
  assert got.batch_size[0] == want.batch_size[0] == 480
  n_kept = 400 - want_counts['split'] - want_counts['prune']
  for k in demo.FIELDS:
    assert torch.equal(got.tensors[k].detach()[:n_kept], want.tensors[k].detach()[:n_kept]), k
  for k in ('rotation', 'alpha_logit', 'feature', 'depths'):      # copies; the depth noise is the same float32 sum
    assert torch.equal(got.tensors[k].detach(), want.tensors[k].detach()), k
  got_state, want_state = got.tensor_state, want.tensor_state
  for name, st in want_state.items():
    for key, t in st.items():
      assert torch.equal(got_state[name][key], t), (name, key)
  assert got.parameter_groups == want.parameter_groups and got.other_state == want.other_state

  # check 2 on the children: replay the draws of uniform_split_gaussians2d(random_axis=True) for the float64 yardstick
  prune_cost, split_score = heuristics
  prune_mask = demo.take_n(prune_cost, int(0.025 * 400 * 0.9), descending=False)
  split_mask = demo.take_n(split_score, max(0, 80 + int(prune_mask.sum())), descending=True)
  split_mask = split_mask & ~prune_mask
  parents = demo.as_gaussians(params).detach()[split_mask]
  torch.manual_seed(42)
  probs = torch.nn.functional.normalize(parents.scaling + 1e-6, p=1, dim=1)
  onehot = torch.nn.functional.one_hot(torch.multinomial(probs, num_samples=1).squeeze(1), num_classes=2)
  steps = torch.linspace(-0.7, 0.7, 2, device=DEV, dtype=torch.float64)
  z = steps.view(1, 2, 1) * onehot.double().view(-1, 1, 2)
  factor = onehot.double() * (math.sqrt(2) / 2) + (1 - onehot.double())
  f64 = split2d_reference(parents, z, factor, 2, torch.float64)
  f32 = split2d_reference(parents, z.float(), factor, 2, torch.float32)
  assert torch.equal(f32.position, want.tensors['position'].detach()[n_kept:]), "the replayed draws are not the run's"
  kernel = {k: got.tensors[k].detach()[n_kept:] for k in ('position', 'log_scaling')}
  deviations(('position', 'log_scaling'), kernel, dict(position=f32.position, log_scaling=f32.log_scaling),
             dict(position=f64.position, log_scaling=f64.log_scaling), "fit, first split_prune")
