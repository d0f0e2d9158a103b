"""Fractional / visibility-aware optimisers.  CPU part: the oracle restatement of the
moment kernels is pinned by the identity with torch.optim.Adam; GPU part: the HIP kernel vs the oracle
and the optimizer classes end to end."""
import ctypes
import math

import pytest
import torch

from oracle import optim as oopt


def test_oracle_adam_with_unit_weights_is_torch_adam():
  torch.manual_seed(0)
  n, d = 50, 3
  p0 = torch.randn(n, d)
  ref = p0.clone().requires_grad_(True)
  opt = torch.optim.Adam([ref], lr=0.01, betas=(0.9, 0.999), eps=1e-16)
  p = p0.clone()
  m, v, tw = torch.zeros(n, d), torch.zeros(n, d), torch.zeros(n)
  idx = torch.arange(n)
  sat = 1 - math.exp(-2.0)
  for it in range(5):
    g = torch.randn(n, d)
    ref.grad = g.clone()
    before = ref.detach().clone()
    opt.step()
    adam_step = before - ref.detach()
    tw += 1.0
    step = oopt.fractional_step(0, False, idx, torch.ones(n), m, v, tw, g, 0.01, (0.9, 0.999), 1e-16, True)
    assert torch.allclose(step, adam_step, rtol=1e-4, atol=5e-7), (step - adam_step).abs().max()
    p -= step * sat
  assert torch.isfinite(p).all()


def _random_case(seed, d, vector):
  torch.manual_seed(seed)
  n, mcount = 1000, 400
  idx = torch.randperm(n)[:mcount].sort().values
  weight = torch.rand(mcount) * 1.5 + 0.01
  m = torch.randn(n, d) * 0.1
  v = (torch.rand(n) if vector else torch.rand(n, d)) * 0.1
  tw = torch.rand(n) * 5 + weight.max()
  grad = torch.randn(n, d)
  return idx, weight, m, v, tw, grad


@pytest.mark.gpu
@pytest.mark.parametrize('kind', [0, 1])
@pytest.mark.parametrize('vector,d', [(False, 1), (False, 3), (False, 48), (True, 3), (True, 4)])
@pytest.mark.parametrize('bias_correction', [True, False])
def test_kernel_matches_oracle(kind, vector, d, bias_correction):
  from taichi_splatting_amd.optim.fractional import fractional_step
  idx, weight, m, v, tw, grad = _random_case(kind * 10 + d, d, vector)
  m_o, v_o = m.clone(), v.clone()
  want = oopt.fractional_step(kind, vector, idx, weight, m_o, v_o, tw, grad, 0.02, (0.9, 0.99), 1e-16, bias_correction)
  dev = 'cuda:0'
  m_g, v_g = m.to(dev), v.to(dev)
  step = torch.zeros(idx.shape[0], d, device=dev)
  fractional_step(kind, vector, step, idx.to(dev), weight.to(dev), m_g, v_g, tw.to(dev), grad.to(dev), 0.02,
                  (0.9, 0.99), 1e-16, bias_correction)
  # float32 pow(beta, w) differs by an ulp between host and device; 1 - beta^w amplifies it ~100x
  assert torch.allclose(step.cpu(), want, rtol=2e-4, atol=1e-6), (step.cpu() - want).abs().max()
  assert torch.allclose(m_g.cpu(), m_o, rtol=2e-4, atol=1e-6)
  assert torch.allclose(v_g.cpu(), v_o, rtol=2e-4, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', [0, 1])
@pytest.mark.parametrize('group_type,d', [('scalar', 1), ('scalar', 3), ('scalar', 16), ('scalar', 48), ('scalar', 100),
                                          ('vector', 1), ('vector', 3), ('vector', 4), ('vector', 48), ('vector', 200),
                                          ('local_vector', 2), ('local_vector', 3)])
@pytest.mark.parametrize('extras', [False, True])
def test_fused_update_matches_oracle(kind, group_type, d, extras):
  # ms_fractional_update (one kernel per group) against the restated host logic of the reference
  from taichi_splatting_amd.optim.fractional import Group, fused_update
  torch.manual_seed(kind * 1000 + d + 7 * extras)
  vector = group_type != 'scalar'
  idx, weight, m, v, tw, grad = _random_case(kind * 10 + d, d, vector)
  n, mc = grad.shape[0], idx.shape[0]
  param = torch.randn(n, d)
  basis = None
  if group_type == 'local_vector':
    q, _ = torch.linalg.qr(torch.randn(mc, d, d))
    basis = q * (torch.rand(mc, 1, d) + 0.3)               # orthogonal axes scaled per column, like point_basis
  grad_scale = torch.rand(mc) + 0.5 if extras else None
  mask_lr = torch.rand(d) if extras else None
  point_lr = torch.rand(n) + 0.5 if extras else None
  clip = 0.7 if extras else None
  if extras:
    grad[idx[0], 0] = float('inf')                           # non-finite steps are dropped
  p_o, m_o, v_o = param.clone(), m.clone(), v.clone()
  oopt.group_update(kind, group_type, p_o, grad, m_o, v_o, idx, weight, tw, 0.02, (0.9, 0.99), 1e-16, True,
                    grad_scale=grad_scale, basis=basis, clip=clip, mask_lr=mask_lr, point_lr=point_lr)
  dev = 'cuda:0'
  g = lambda t: t.to(dev) if t is not None else None
  p_g = param.to(dev)
  # state naming quirk of the reference: for vector groups state['v'] is the (N, D) first moment
  state = {'v': m.to(dev), 'm': v.to(dev)}
  group = Group(name='p', type=group_type, param=p_g, grad=g(grad), state=state, lr=0.02, betas=(0.9, 0.99), eps=1e-16,
                bias_correction=True, clip=clip, mask_lr=g(mask_lr), point_lr=g(point_lr))
  fused_update(group, g(weight), g(idx), g(tw), kind, g(basis), grad_scale=g(grad_scale))
  keep = torch.ones(n, dtype=torch.bool)
  if extras:
    keep[idx[0]] = False                                      # the row fed with inf: only "finite" is required
    assert torch.isfinite(p_g.cpu()[idx[0]]).all()
  assert torch.allclose(p_g.cpu()[keep], p_o[keep], rtol=3e-4, atol=2e-6), (p_g.cpu() - p_o)[keep].abs().max()
  assert torch.allclose(state['v'].cpu()[keep], m_o[keep], rtol=3e-4, atol=2e-6)
  assert torch.allclose(state['m'].cpu()[keep], v_o[keep], rtol=3e-4, atol=2e-6)
  untouched = torch.ones(n, dtype=torch.bool); untouched[idx] = False
  assert torch.equal(p_g.cpu()[untouched], param[untouched])


@pytest.mark.gpu
def test_optimizer_classes_end_to_end():
  from taichi_splatting_amd.optim import (FractionalAdam, SparseLaProp, VisibilityAwareAdam, ParameterClass)
  dev = 'cuda:0'
  torch.manual_seed(0)
  n = 500
  tensors = dict(position=torch.randn(n, 3, device=dev), feature=torch.randn(n, 3, 4, device=dev),
                 label=torch.arange(n, device=dev))
  groups = dict(position=dict(lr=0.01, type='vector'), feature=dict(lr=0.02, type='scalar'))
  params = ParameterClass(tensors, groups, optimizer=VisibilityAwareAdam, vis_beta=0.5)
  target = torch.zeros(n, 3, device=dev)
  first = None
  for it in range(30):
    params.zero_grad()
    loss = ((params.position - target) ** 2).sum() + (params.feature ** 2).sum()
    loss.backward()
    idx = torch.arange(0, n, 2, device=dev)
    vis = torch.rand(idx.shape[0], device=dev) + 0.1
    params.step(indexes=idx, visibility=vis)
    first = first if first is not None else float(loss)
  assert float(loss) < first
  # only the visible (even) rows moved
  assert torch.equal(params.position.detach()[1::2], tensors['position'][1::2])
  # filtering / appending keeps the optimizer state aligned
  sub = params[torch.arange(0, 100, device=dev)]
  assert sub.batch_size == (100,) and sub.tensor_state['position']['total_weight'].shape == (100,)
  more = sub.append_tensors({k: v.detach()[:10] for k, v in sub.tensors.items()})
  assert more.batch_size == (110,) and more.tensor_state['feature']['m'].shape[0] == 110
  assert set(params.learning_rates) == {'position', 'feature'}
  params.set_learning_rate(position=0.5)
  assert params.learning_rates['position'] == 0.5

  # the plain fractional optimisers
  for cls, kw in ((FractionalAdam, dict(weight=True)), (SparseLaProp, dict(weight=False))):
    p = torch.nn.Parameter(torch.randn(200, 3, device=dev))
    opt = cls([dict(params=[p], name='p', type='scalar')], lr=0.05)
    before = float((p ** 2).sum())
    for _ in range(20):
      opt.zero_grad()
      (p ** 2).sum().backward()
      idx = torch.arange(200, device=dev)
      if kw['weight']:
        opt.step(idx, torch.full((200,), 0.7, device=dev))
      else:
        opt.step(idx)
    assert float((p ** 2).sum()) < before


FIVE_GROUPS = [('position', 'scalar', 3), ('log_scaling', 'vector', 3), ('rotation', 'scalar', 4), ('alpha_logit', 'scalar', 1),
               ('feature', 'vector', 48), ('sh', 'scalar', 48), ('offset', 'local_vector', 3), ('wide', 'scalar', 12)]


def _five_group_case(seed, n=3000, mcount=1700, unaligned=False):
  torch.manual_seed(seed)
  idx = torch.randperm(n)[:mcount].sort().values
  weight = torch.rand(mcount) * 1.5 + 0.01
  tw = torch.rand(n) * 5 + weight.max()
  groups = {}
  for name, kind, d in FIVE_GROUPS:
    groups[name] = dict(type=kind, d=d, param=torch.randn(n, d), grad=torch.randn(n, d), m=torch.randn(n, d) * 0.1,
                        v=(torch.rand(n, d) if kind == 'scalar' else torch.rand(n)) * 0.1)
  q, _ = torch.linalg.qr(torch.randn(mcount, 3, 3))
  basis = q * (torch.rand(mcount, 1, 3) + 0.3)
  return idx, weight, tw, groups, basis


@pytest.mark.gpu
@pytest.mark.parametrize('kind', [0, 1])
@pytest.mark.parametrize('dense', [False, True])
def test_all_groups_in_one_launch_match_the_oracle(kind, dense):
  """ms_optim_step_groups: eight groups (rows of 3 / 3 / 4 / 1 / 48 / 48 / 3 / 12 floats; scalar, vector and local_vector;
  16-byte pieces where the row length allows) in one launch against the restated host logic, group by group — with a
  sparse index list and in the dense mode (row i = point i, negative weights skip)."""
  from taichi_splatting_amd.optim.fractional import Group, fused_update_groups
  idx, weight, tw, groups, basis = _five_group_case(31 + kind)
  n, mc = tw.shape[0], idx.shape[0]
  grad_scale = torch.rand(mc) + 0.5
  want = {}
  for name, g in groups.items():
    p_o, m_o, v_o = g['param'].clone(), g['m'].clone(), g['v'].clone()
    oopt.group_update(kind, g['type'], p_o, g['grad'], m_o, v_o, idx, weight, tw, 0.02, (0.9, 0.99), 1e-16, True,
                      grad_scale=grad_scale, basis=basis if g['type'] == 'local_vector' else None, clip=0.9)
    want[name] = (p_o, m_o, v_o)
  dev = 'cuda:0'
  if dense:
    w_full, gs_full, basis_full = torch.full((n,), -1.0), torch.zeros(n), torch.zeros(n, 3, 3)
    w_full[idx], gs_full[idx], basis_full[idx] = weight, grad_scale, basis
    args = (w_full.to(dev), None, tw.to(dev))
    extra = dict(basis=basis_full.to(dev), grad_scale=gs_full.to(dev))
  else:
    args = (weight.to(dev), idx.to(dev), tw.to(dev))
    extra = dict(basis=basis.to(dev), grad_scale=grad_scale.to(dev))
  states, objs = {}, []
  for name, g in groups.items():
    states[name] = {'v': g['m'].to(dev), 'm': g['v'].to(dev)}      # (the reference's naming quirk: 'v' is the first moment)
    objs.append(Group(name=name, type=g['type'], param=g['param'].to(dev), grad=g['grad'].to(dev), state=states[name], lr=0.02,
                      betas=(0.9, 0.99), eps=1e-16, bias_correction=True, clip=0.9, mask_lr=None, point_lr=None))
  fused_update_groups(objs, args[0], args[1], args[2], kind, **extra)
  untouched = torch.ones(n, dtype=torch.bool); untouched[idx] = False
  for obj in objs:
    p_o, m_o, v_o = want[obj.name]
    assert torch.allclose(obj.param.cpu(), p_o, rtol=3e-4, atol=2e-6), (obj.name, (obj.param.cpu() - p_o).abs().max())
    assert torch.allclose(states[obj.name]['v'].cpu(), m_o, rtol=3e-4, atol=2e-6), obj.name
    assert torch.allclose(states[obj.name]['m'].cpu(), v_o, rtol=3e-4, atol=2e-6), obj.name
    assert torch.equal(obj.param.cpu()[untouched], groups[obj.name]['param'][untouched]), obj.name


@pytest.mark.gpu
def test_visibility_weights_kernel_matches_the_oracle_and_dense_mode_skips():
  from taichi_splatting_amd import _lib
  lib = _lib.load()
  dev = 'cuda:0'
  torch.manual_seed(3)
  n = 5000
  vis_full = torch.rand(n) * (torch.rand(n) > 0.4)                 # 40 % invisible
  vis_full[:7] = 1e-8                                               # exactly at the threshold: invisible in the dense mode
  idx = (vis_full > 1e-8).nonzero().squeeze(1)
  running, tw = torch.rand(n), torch.rand(n) * 3
  running[idx[::5]] = 0.0                                           # a point's first step: no running visibility yet
  # the float64 oracle on the float32 inputs
  r_o, tw_o = running.double(), tw.double()
  w_o, gs_o = oopt.visibility_weights(r_o, vis_full[idx].double(), idx, tw_o, 0.8, 0.1)
  stream = _lib.current_stream(torch.device(dev))
  # sparse
  r_g, tw_g = running.to(dev), tw.to(dev)
  w_g, gs_g = torch.empty(idx.shape[0], device=dev), torch.empty(idx.shape[0], device=dev)
  idx_g, vis_g, vis_full_g = idx.to(dev), vis_full[idx].to(dev), vis_full.to(dev)      # (alive across the launches)
  _lib.check(lib.ms_optim_visibility_weights(idx_g.data_ptr(), vis_g.data_ptr(), idx.shape[0], 0.8, 0.1,
                                             1e-12, 1e-8, r_g.data_ptr(), tw_g.data_ptr(), w_g.data_ptr(), gs_g.data_ptr(), stream), "w")
  for got, want in ((r_g, r_o), (tw_g, tw_o), (w_g, w_o), (gs_g, gs_o)):
    assert torch.allclose(got.cpu().double(), want, rtol=2e-6, atol=1e-7), (got.cpu().double() - want).abs().max()
  # dense: same state, weights at the visible rows, -1 elsewhere, invisible rows untouched
  r_d, tw_d = running.to(dev), tw.to(dev)
  w_d, gs_d = torch.empty(n, device=dev), torch.empty(n, device=dev)
  _lib.check(lib.ms_optim_visibility_weights(None, vis_full_g.data_ptr(), n, 0.8, 0.1, 1e-12, 1e-8, r_d.data_ptr(),
                                             tw_d.data_ptr(), w_d.data_ptr(), gs_d.data_ptr(), stream), "w dense")
  assert torch.equal(r_d, r_g) and torch.equal(tw_d, tw_g)
  assert torch.equal(w_d.cpu()[idx], w_g.cpu())
  hidden = torch.ones(n, dtype=torch.bool); hidden[idx] = False
  assert bool((w_d.cpu()[hidden] == -1).all()) and torch.equal(r_d.cpu()[hidden], running[hidden])
  assert torch.equal(tw_d.cpu()[hidden], tw[hidden]) and bool((gs_d.cpu()[hidden] == 0).all())
  assert bool((w_d.cpu()[:7] == -1).all())


@pytest.mark.gpu
def test_visibility_weights_edges_on_the_index_list():
  """Zero visibility on the index list (weight 0, the running visibility decays), zero running visibility with zero
  visibility (0 / max(0, floor) = 0), and a visibility exactly at the skip threshold (listed: updated) against the
  float64 oracle."""
  from taichi_splatting_amd import _lib
  lib = _lib.load()
  torch.manual_seed(4)
  n, mc = 1000, 300
  idx = torch.randperm(n)[:mc]
  vis = torch.rand(mc)
  vis[:40] = 0.0
  vis[40:50] = 1e-8
  running, tw = torch.rand(n), torch.rand(n) * 3
  running[idx[20:60]] = 0.0
  r_o, tw_o = running.double(), tw.double()
  w_o, gs_o = oopt.visibility_weights(r_o, vis.double(), idx, tw_o, 0.8, 0.1)
  r_g, tw_g, idx_g, vis_g = running.to(DEV), tw.to(DEV), idx.to(DEV), vis.to(DEV)
  w_g, gs_g = torch.full((mc,), float('nan'), device=DEV), torch.full((mc,), float('nan'), device=DEV)
  _lib.check(lib.ms_optim_visibility_weights(idx_g.data_ptr(), vis_g.data_ptr(), mc, 0.8, 0.1, 1e-12, 1e-8, r_g.data_ptr(),
                                             tw_g.data_ptr(), w_g.data_ptr(), gs_g.data_ptr(),
                                             _lib.current_stream(torch.device(DEV))), "w edges")
  for got, want in ((r_g, r_o), (tw_g, tw_o), (w_g, w_o), (gs_g, gs_o)):
    assert torch.allclose(got.cpu().double(), want, rtol=2e-6, atol=1e-7), (got.cpu().double() - want).abs().max()
  assert bool((w_g.cpu()[:40] == 0).all()) and bool((w_g.cpu()[40:50] > 0).all())
  assert torch.equal(tw_g.cpu()[idx[:40]], tw[idx[:40]])


@pytest.mark.gpu
def test_visibility_aware_dense_step_equals_the_indexed_step():
  """``step(None, visibility_of_every_point)`` (no torch.nonzero, no host synchronisation) leaves parameters and
  optimiser state bit for bit where ``step(visible, visibility[visible])`` of the reference's loop leaves them."""
  from taichi_splatting_amd.optim import ParameterClass, VisibilityAwareAdam
  dev = 'cuda:0'
  torch.manual_seed(0)
  n = 4000
  base = dict(position=torch.randn(n, 3), log_scaling=torch.randn(n, 3), rotation=torch.randn(n, 4), alpha_logit=torch.randn(n, 1),
              feature=torch.randn(n, 3, 16))
  groups = dict(position=dict(lr=0.01), log_scaling=dict(lr=0.02, type='vector'), rotation=dict(lr=0.01), alpha_logit=dict(lr=0.05),
                feature=dict(lr=0.02, type='vector'))
  results = []
  for dense in (False, True):
    params = ParameterClass({k: v.clone().to(dev) for k, v in base.items()}, groups, optimizer=VisibilityAwareAdam, vis_beta=0.8,
                            vis_smooth=0.1, betas=(0.9, 0.95))
    torch.manual_seed(1)
    for it in range(4):
      params.zero_grad()
      loss = sum((t ** 2).sum() * (i + 1) for i, t in enumerate(params.tensors.values()))
      loss.backward()
      vis = (torch.rand(n, device=dev) * (torch.rand(n, device=dev) > 0.3)).contiguous()
      if dense:
        params.step(indexes=None, visibility=vis)
      else:
        visible = (vis > 1e-8).nonzero().squeeze(1)
        params.step(indexes=visible, visibility=vis[visible])
    results.append(({k: v.detach().clone() for k, v in params.tensors.items()}, params.tensor_state))
  (pa, sa), (pb, sb) = results
  for k in pa:
    assert torch.equal(pa[k], pb[k]), k
    for key in sa[k]:
      assert torch.equal(sa[k][key], sb[k][key]), (k, key)


# ================================================================================================================
# The kernels against a float64 oracle, with an error model instead of a flat tolerance.
#
# The kernels compute in float32; the oracle (oracle/optim.py, dtype-generic) runs on float64 copies of the same
# float32 inputs.  An output element is accepted when
#     |got - want| <= C_TOL * 2^-24 * kappa_row * S_elem
#   S_elem     the oracle's own output on absolute values (|m|, |g|, |param|, |grad_scale| ...): a running error scale,
#              so that what cancels inside lerp(t, m, g) or in param - step is still charged for (a row with a negative
#              weight has beta^w > 1 and 1 - beta^w < 0: its gradient goes in as -|g|, so that the lerp still adds);
#   kappa_row  how much the per-point factors amplify float32 rounding.  The kernel makes beta^t as exp2(t log2 beta),
#              with a relative error of (1 + 2 t |ln beta|) ulp (the exp2, the rounded log2 beta and product), and
#              1 - beta^t turns that into beta^t (1 + 2 t |ln beta|) / |1 - beta^t| ulp: about 1000 for beta2 = 0.999
#              and t = 1, and ~1 / (t |ln beta|) for small t — the first step of a point with a small weight is ill
#              conditioned in float32, in the reference's float32 kernels as well.  Summed over beta1, beta2 and
#              t = w (the lerps), t = tw (the bias corrections, when on), plus the saturation 1 - exp(-2 w) (the same
#              function of w with beta = e^-2); vector groups add sqrt(d) for the rounding of their squared norm, a
#              sum of d positive terms (random-walk estimate; the kernels sum at most 16 terms per lane, then a tree).
#   C_TOL = 32 the longest chain of plainly rounded operations behind one output (LaProp into param: lerp 3, sqrt and
#              divisions 3, lr / bias1 2, mask and point lr 2, saturation product and subtraction 2, plus v_exp_f32 /
#              v_sqrt_f32 within 1 ulp each) is about 16 roundings of at most 1 ulp of the running scale: twice that.
#              test_tolerance_catches_mutated_oracles shows that seven plausible kernel mistakes still exceed it.
# ================================================================================================================
U = 2.0 ** -24
C_TOL = 32
TINY = 2.0 ** -126                          # (float32 subnormal range: an absolute floor)
LR, BETAS, EPS = 0.02, (0.9, 0.999), 1e-16
MS_ERR_BAD_ARG, MS_ERR_ABI = -1, -4

# row lengths of the sweep; ms_fractional_step also takes rows wider than 256 floats (thread-per-point kernel)
D_SWEEP = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 27, 45, 48, 63, 64, 65, 127, 255, 256)
D_WIDE = (257, 300)
D_MISALIGNED = (4, 16, 48, 100)

# Shape (csrc/optim.hip, pick_shape) -> template arguments <LPP, KMAX, VEC> of fractional_update_kernel, and the cases of
# the sweep that reach it (every group type and kind; local_vector rows always take <4, 1, 1>).  Checked once with a
# kernel trace of the sweep; test_sweep_reaches_every_row_shape checks the table against the restated rule below.
SHAPES = {  # Shape: (<LPP, KMAX, VEC>, aligned d of D_SWEEP, d of D_MISALIGNED with one array misaligned)
  'S_V1_L1': ((1, 1, 1), (1,), ()),
  'S_V1_L4': ((4, 1, 1), (2, 3), (4,)),                # and local_vector d = 2, 3
  'S_V1_L16': ((16, 1, 1), (5, 7, 15), (16,)),
  'S_V1_L16_K4': ((16, 4, 1), (17, 27, 45, 63), (48,)),
  'S_V1_L16_K16': ((16, 16, 1), (65, 127, 255), (100,)),
  'S_V4_L1': ((1, 1, 4), (4,), ()),
  'S_V4_L4': ((4, 1, 4), (8, 16), ()),
  'S_V4_L16': ((16, 1, 4), (48, 64), ()),
  'S_V4_L16_K4': ((16, 4, 4), (256,), ()),
}


def _pick_shape(d, aligned=True, local_vector=False):
  """pick_shape of csrc/optim.hip, restated."""
  if local_vector:
    return 'S_V1_L4'
  if d % 4 == 0 and aligned:
    return 'S_V4_L1' if d == 4 else 'S_V4_L4' if d <= 16 else 'S_V4_L16' if d <= 64 else 'S_V4_L16_K4'
  return 'S_V1_L1' if d == 1 else 'S_V1_L4' if d <= 4 else 'S_V1_L16' if d <= 16 else 'S_V1_L16_K4' if d <= 64 else 'S_V1_L16_K16'


def _cond_pow(beta, t):
  """Rounding amplification (in ulp) of 1 - beta^t made in float32 as 1 - exp2(t log2 beta), elementwise over t."""
  t = t.double()
  if beta == 0.0:
    return torch.zeros_like(t)                          # beta^t is exactly 0 (t > 0) or 1 (t = 0: pow_beta)
  bt = torch.tensor(beta, dtype=torch.float64) ** t
  k = bt * (1 + 2 * t.abs() * abs(math.log(beta))) / (1 - bt).abs()
  return torch.where(t == 0, torch.zeros_like(k), k)   # beta^0 = 1 exactly


def _kappa(w, tw, betas, bias_correction, vector, d):
  """kappa_row (M,) for the visible rows: w (M,), tw (M,) = total_weight[indexes]."""
  k = 1.0 + _cond_pow(math.exp(-2.0), w)
  for beta in betas:
    k = k + _cond_pow(beta, w)
    if bias_correction:
      k = k + _cond_pow(beta, tw)
  return k + (math.sqrt(d) if vector else 0.0)


def _f64(t, f=None):
  if t is None:
    return None
  t = t.double().clone()
  return f(t) if f is not None else t


def _hp(**kw):
  hp = dict(lr=LR, betas=BETAS, eps=EPS, bias_correction=True, clip=None)
  hp.update(kw)
  return hp


def _oracle(entry, kind, gtype, c, hp, mutation=None):
  """float64 oracle of one group: entry 'step' (ms_fractional_step: the raw step) or 'update' (ms_fractional_update /
  ms_optim_step_groups: param, moments).  Returns (want, scale, kappa): dicts of the outputs at the visible rows
  (step (M, d), param (M, d), m (M, d), v (M, d) or (M,)) and kappa (M,)."""
  idx, d = c['idx'], c['grad'].shape[1]
  vector = gtype != 'scalar'
  w, tw = c['w'].double(), c['tw'].double()
  args = (idx, w, tw, hp['lr'], hp['betas'], hp['eps'], hp['bias_correction'])
  want, scale = {}, {}
  sign = torch.where(w < 0, -1.0, 1.0).to(torch.float64).unsqueeze(1)
  g_abs = _f64(c['grad'], torch.abs)
  g_abs[idx] = g_abs[idx] * sign
  if entry == 'step':
    m, v = _f64(c['m']), _f64(c['v'])
    want['step'] = oopt.fractional_step(kind, vector, idx, w, m, v, tw, _f64(c['grad']), hp['lr'], hp['betas'],
                                        hp['eps'], hp['bias_correction'], mutation)
    want['m'], want['v'] = m[idx], v[idx]
    m, v = _f64(c['m'], torch.abs), _f64(c['v'])
    scale['step'] = oopt.fractional_step(kind, vector, idx, w, m, v, tw, g_abs, hp['lr'], hp['betas'], hp['eps'],
                                         hp['bias_correction']).abs()
    scale['m'], scale['v'] = m[idx].abs(), v[idx]
  else:
    p, m, v = _f64(c['param']), _f64(c['m']), _f64(c['v'])
    extra = dict(grad_scale=_f64(c['gs']), basis=_f64(c['basis']), clip=hp['clip'], mask_lr=_f64(c['mask']),
                 point_lr=_f64(c['plr']), mutation=mutation)
    oopt.group_update(kind, gtype, p, _f64(c['grad']), m, v, *args, **extra)
    want['param'], want['m'], want['v'] = p[idx], m[idx], v[idx]
    # the scale: every input by its magnitude; local_vector rows through |B^-1| and |B|
    g = g_abs
    gs = _f64(c['gs'], torch.abs)
    if gs is not None:
      g[idx] = g[idx] * gs.unsqueeze(1)
    if gtype == 'local_vector':
      B = c['basis'].double()
      g[idx] = torch.einsum('bij,bj->bi', torch.linalg.inv(B).abs(), g[idx])
    m, v = _f64(c['m'], torch.abs), _f64(c['v'])
    s = oopt.group_update(kind, 'vector' if vector else 'scalar', _f64(c['param']), g, m, v, *args,
                          clip=hp['clip'], point_lr=_f64(c['plr'], torch.abs)).abs()
    if gtype == 'local_vector':
      s = torch.einsum('bij,bj->bi', B.abs(), s)
    if c['mask'] is not None:
      s = s * c['mask'].double().abs().unsqueeze(0)
    sat = (1 - torch.exp(-2 * w)).abs().unsqueeze(1)
    scale['param'] = c['param'].double().abs()[idx] + s * sat
    scale['m'], scale['v'] = m[idx].abs(), v[idx]
  return want, scale, _kappa(w, tw[idx], hp['betas'], hp['bias_correction'], vector, d)


def _excess(got, want, scale, kappa):
  """Boolean mask of the elements outside the error model (non-finite values must match exactly: NaN for NaN, inf of
  the same sign)."""
  got, want = got.detach().cpu().double(), want.double()
  assert got.shape == want.shape, (got.shape, want.shape)
  k = kappa.view(-1, *([1] * (want.dim() - 1)))
  tol = C_TOL * U * k * scale + TINY
  fin = torch.isfinite(want)
  out = ~fin & ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
  out |= fin & ~((got - want).abs() <= tol)           # (a NaN tolerance or a non-finite got counts as outside)
  return out


def _assert_outputs(what, got, want, scale, kappa):
  for key in want:
    bad = _excess(got[key], want[key], scale[key], kappa)
    if bad.any():
      i = bad.nonzero()[0].tolist()
      g = got[key].detach().cpu().double()[tuple(i)]
      raise AssertionError(f"{what} {key}: {int(bad.sum())} of {bad.numel()} elements outside the error model, first at "
                           f"{i}: got {float(g)!r}, want {float(want[key][tuple(i)])!r}, scale {float(scale[key][tuple(i)]):.3e}, "
                           f"kappa {float(kappa[i[0]]):.3e}")


def _arrays(gen, n, d, gtype, mc=None):
  r = lambda *s: torch.rand(*s, generator=gen)
  out = dict(param=torch.randn(n, d, generator=gen), grad=torch.randn(n, d, generator=gen),
             m=torch.randn(n, d, generator=gen) * 0.1, v=(r(n) if gtype != 'scalar' else r(n, d)) * 0.1, basis=None)
  if gtype == 'local_vector':
    q, _ = torch.linalg.qr(torch.randn(mc, d, d, generator=gen))
    out['basis'] = (q * (r(mc, 1, d) + 0.3)).contiguous()     # orthogonal axes scaled per column, like point_basis
  return out


def _common(gen, n, mc):
  """Visible rows: a count that is not a multiple of 256, unsorted; tw is the total weight after this step's weight."""
  idx = torch.randperm(n, generator=gen)[:mc]
  w = torch.rand(mc, generator=gen) * 1.5 + 0.01
  tw = torch.rand(n, generator=gen) * 5
  tw[idx] += w
  return dict(idx=idx, w=w, tw=tw, gs=None, mask=None, plr=None)


def _case(seed, d, gtype, n=700, mc=300):
  gen = torch.Generator().manual_seed(seed)
  c = _common(gen, n, mc)
  c.update(_arrays(gen, n, d, gtype, mc))
  return c


def _sweep_cases():
  """(entry, kind, group type, case, hyper-parameters) of the row-length sweep."""
  for d in D_SWEEP + D_WIDE:
    for kind in (0, 1):
      for gtype in ('scalar', 'vector'):
        for bc in (True, False):
          c = _case(1000 * d + 100 * kind + 10 * (gtype == 'vector') + bc, d, gtype)
          yield 'step', kind, gtype, c, _hp(bias_correction=bc)
          if d <= 256:
            yield 'update', kind, gtype, c, _hp(bias_correction=bc)
  for d in (2, 3):
    for kind in (0, 1):
      yield 'update', kind, 'local_vector', _case(77 + d + kind, d, 'local_vector'), _hp()


# edge rows: (w, tw) pairs, one per row, cycling; betas; clamps
EDGE_WEIGHTS = [(w, tw) for w in (0.0, 1e-3, 1.0, 50.0, 200.0) for tw in (w, w + 20.0)] + [(0.0, 0.0)]
EDGE_BETAS = ((0.0, 0.5), (0.9, 0.999), (0.99, 0.9999))
EDGE_NONFINITE = (float('inf'), float('-inf'), float('nan'))


def _edge_case(seed, d, gtype, clamps, n=400, mc=264):
  gen = torch.Generator().manual_seed(seed)
  idx = torch.randperm(n, generator=gen)[:mc]
  pairs = torch.tensor([EDGE_WEIGHTS[i % len(EDGE_WEIGHTS)] for i in range(mc)], dtype=torch.float32)
  w = pairs[:, 0].contiguous()
  tw = torch.rand(n, generator=gen) * 5
  tw[idx] = pairs[:, 1]
  c = dict(idx=idx, w=w, tw=tw, gs=None, mask=None, plr=None)
  c.update(_arrays(gen, n, d, gtype, mc))
  c['m'][idx[:mc // 2]] = 0.0                            # first steps: nothing accumulated yet
  c['v'][idx[:mc // 2]] = 0.0
  # non-finite gradient elements: rows 5, 6, 7 of every 24 (every weight pair meets each of them)
  for j in range(mc):
    if j % 24 in (5, 6, 7):
      c['grad'][idx[j], j % d] = EDGE_NONFINITE[j % 24 - 5]
  if clamps:
    c['gs'] = torch.rand(mc, generator=gen) * 4 + 0.1               # a gradient scale of up to 4
    c['mask'] = torch.rand(d, generator=gen)
    c['mask'][0] = 0.0
    c['plr'] = torch.rand(n, generator=gen) * 2
  return c


def _edge_cases():
  for bi, betas in enumerate(EDGE_BETAS):
    for kind in (0, 1):
      for gtype in ('scalar', 'vector'):
        for clamps in (False, True):
          c = _edge_case(bi * 8 + kind * 4 + (gtype == 'vector') * 2 + clamps, 3 if gtype == 'scalar' else 5, gtype, clamps)
          # clamps: eps 1e-3 binds where the second moment is small, clip 0.5 binds on most rows
          hp = _hp(betas=betas, eps=1e-3, clip=0.5) if clamps else _hp(betas=betas)
          yield ('update', kind, gtype, c, hp)
          if not clamps:
            yield ('step', kind, gtype, c, hp)


def test_oracle_runs_in_the_dtype_of_its_inputs():
  c = _case(5, 6, 'vector')
  c['gs'], c['mask'], c['plr'] = torch.rand(300) + 0.5, torch.rand(6), torch.rand(700)
  want, scale, kappa = _oracle('update', 1, 'vector', c, _hp(clip=0.5))
  for t in list(want.values()) + list(scale.values()) + [kappa]:
    assert t.dtype == torch.float64
  p, m, v = c['param'].clone(), c['m'].clone(), c['v'].clone()
  oopt.group_update(1, 'vector', p, c['grad'], m, v, c['idx'], c['w'], c['tw'], LR, BETAS, EPS, True, grad_scale=c['gs'],
                    clip=0.5, mask_lr=c['mask'], point_lr=c['plr'])
  want32 = dict(param=p[c['idx']], m=m[c['idx']], v=v[c['idx']])
  assert all(t.dtype == torch.float32 for t in want32.values())
  # float32 inputs stay float32: the two runs differ, by float32 rounding
  assert any(not torch.equal(want32[k].double(), want[k]) for k in want)


def test_oracle_max_with_eps_ignores_nan_like_fmaxf():
  # a NaN gradient element in a vector row: v is NaN, the scale lr / eps, the other elements a finite step
  idx, w = torch.tensor([0]), torch.tensor([1.0], dtype=torch.float64)
  g = torch.tensor([[1.0, float('nan'), 2.0]], dtype=torch.float64)
  m, v = torch.zeros(1, 3, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
  step = oopt.fractional_step(0, True, idx, w, m, v, torch.ones(1, dtype=torch.float64), g, 1.0, (0.5, 0.5), 1e-3, False)
  assert torch.isnan(v).all() and torch.isnan(step[0, 1])
  assert torch.equal(step[0, [0, 2]], torch.tensor([0.5, 1.0], dtype=torch.float64) / 1e-3)


def _float32_oracle(entry, kind, gtype, c, hp):
  idx = c['idx']
  vector = gtype != 'scalar'
  p, m, v = c['param'].clone(), c['m'].clone(), c['v'].clone()
  if entry == 'step':
    s = oopt.fractional_step(kind, vector, idx, c['w'], m, v, c['tw'], c['grad'], hp['lr'], hp['betas'], hp['eps'],
                             hp['bias_correction'])
    return dict(step=s, m=m[idx], v=v[idx])
  oopt.group_update(kind, gtype, p, c['grad'], m, v, idx, c['w'], c['tw'], hp['lr'], hp['betas'], hp['eps'],
                    hp['bias_correction'], grad_scale=c['gs'], basis=c['basis'], clip=hp['clip'], mask_lr=c['mask'],
                    point_lr=c['plr'])
  return dict(param=p[idx], m=m[idx], v=v[idx])


def test_error_model_admits_the_float32_oracle():
  """The same computation in float32 (on the CPU) lies within the error model of the float64 oracle: the tolerance is
  not tighter than float32 arithmetic allows.  (The edge rows need the kernel's exp2 / pow_beta and are left to the GPU
  test; the non-finite patterns are compared there too.)"""
  for n, (entry, kind, gtype, c, hp) in enumerate(_sweep_cases()):
    if n % 3:
      continue                                        # a third of the sweep keeps the CPU suite quick
    want, scale, kappa = _oracle(entry, kind, gtype, c, hp)
    _assert_outputs(f"float32 oracle {entry} kind {kind} {gtype} d {c['grad'].shape[1]}", _float32_oracle(entry, kind, gtype, c, hp),
                    want, scale, kappa)


MUTATIONS = ('swap_betas', 'bias2_no_sqrt', 'tw_before_step', 'no_saturation', 'grad_scale_on_step', 'mask_before_clip',
             'vector_norm_mean')


def test_tolerance_catches_mutated_oracles():
  """Seven plausible kernel mistakes, each as a mutated oracle on the inputs of the GPU tests: every one of them leaves
  the error model on at least one element."""
  cases = [x for i, x in enumerate(_sweep_cases()) if i % 7 == 0] + list(_edge_cases())
  caught = {}
  for entry, kind, gtype, c, hp in cases:
    want, scale, kappa = _oracle(entry, kind, gtype, c, hp)
    for mutation in MUTATIONS:
      if mutation in caught:
        continue
      bad, _, _ = _oracle(entry, kind, gtype, c, hp, mutation=mutation)
      if any(_excess(bad[k], want[k], scale[k], kappa).any() for k in want):
        caught[mutation] = (entry, kind, gtype, c['grad'].shape[1])
    if len(caught) == len(MUTATIONS):
      break
  assert set(caught) == set(MUTATIONS), f"not caught: {set(MUTATIONS) - set(caught)}"


def test_sweep_reaches_every_row_shape():
  assert _pick_shape(3, local_vector=True) == 'S_V1_L4'
  for name, (_, aligned, misaligned) in SHAPES.items():
    assert all(_pick_shape(d) == name for d in aligned), name
    assert all(_pick_shape(d, aligned=False) == name for d in misaligned), name
  assert sorted(d for _, a, _ in SHAPES.values() for d in a) == sorted(D_SWEEP)
  assert sorted(d for _, _, m in SHAPES.values() for d in m) == sorted(D_MISALIGNED)


# ---- the kernels, through the C ABI directly (misaligned views, NaN-filled outputs, bad group lists) ------------------
DEV = 'cuda:0'


def _gpu(t, misalign=False):
  """t on the GPU; misalign: a contiguous view 4 bytes past a 16-byte boundary."""
  if t is None:
    return None
  if not misalign:
    return t.to(DEV).contiguous()
  out = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)[1:].view(t.shape)
  out.copy_(t.to(DEV))
  assert out.data_ptr() % 16 == 4
  return out


def _ptr(t):
  return None if t is None else t.data_ptr()


def _lib_check(rc, what):
  from taichi_splatting_amd import _lib
  assert rc == 0, f"{what}: rc {rc}: {_lib.load().ms_last_error_string().decode()}"


def _run(entry, kind, gtype, c, hp, misalign=()):
  """ms_fractional_step / ms_fractional_update on c; returns the full-size outputs (param / step, m, v) on the GPU."""
  from taichi_splatting_amd import _lib
  lib = _lib.load()
  d, mc = c['grad'].shape[1], c['idx'].shape[0]
  t = {k: _gpu(c[k], k in misalign) for k in ('param', 'grad', 'm', 'v', 'idx', 'w', 'tw', 'gs', 'basis', 'mask', 'plr')}
  stream = _lib.current_stream(torch.device(DEV))
  b1, b2 = hp['betas']
  if entry == 'step':
    out = _gpu(torch.full((mc, d), float('nan')), 'out_step' in misalign)
    _lib_check(lib.ms_fractional_step(kind, int(gtype != 'scalar'), out.data_ptr(), _ptr(t['idx']), _ptr(t['w']), _ptr(t['m']),
                                      _ptr(t['v']), _ptr(t['tw']), _ptr(t['grad']), mc, d, hp['lr'], b1, b2, hp['eps'],
                                      int(hp['bias_correction']), stream), "ms_fractional_step")
    return dict(step=out, m=t['m'], v=t['v'])
  _lib_check(lib.ms_fractional_update(kind, oopt_group_type(gtype), _ptr(t['param']), _ptr(t['grad']), _ptr(t['m']), _ptr(t['v']),
                                      _ptr(t['idx']), _ptr(t['w']), _ptr(t['tw']), _ptr(t['gs']), _ptr(t['basis']),
                                      _ptr(t['mask']), _ptr(t['plr']), mc, d, hp['lr'], b1, b2, hp['eps'],
                                      hp['clip'] if hp['clip'] is not None else -1.0, int(hp['bias_correction']), stream),
             "ms_fractional_update")
  return dict(param=t['param'], m=t['m'], v=t['v'])


def oopt_group_type(gtype):
  return {'scalar': 0, 'vector': 1, 'local_vector': 2}[gtype]


def _check_run(what, entry, kind, gtype, c, hp, got):
  """got (full-size GPU outputs) against the float64 oracle at the visible rows, and bit for bit untouched elsewhere."""
  idx = c['idx']
  want, scale, kappa = _oracle(entry, kind, gtype, c, hp)
  _assert_outputs(what, {k: got[k].cpu()[idx] if k != 'step' else got[k] for k in want}, want, scale, kappa)
  rest = torch.ones(c['tw'].shape[0], dtype=torch.bool)
  rest[idx] = False
  for k in ('param', 'm', 'v'):
    if k in got:
      assert torch.equal(got[k].cpu()[rest], c[k][rest]), f"{what} {k}: rows outside the index list changed"


@pytest.mark.gpu
def test_every_row_length_against_the_float64_oracle():
  """ms_fractional_step (d up to 300: the thread-per-point kernel past 256) and ms_fractional_update, Adam and LaProp,
  scalar / vector / local_vector, bias correction on and off, 300 unsorted visible rows of 700."""
  for entry, kind, gtype, c, hp in _sweep_cases():
    what = f"{entry} kind {kind} {gtype} d {c['grad'].shape[1]} bc {hp['bias_correction']}"
    _check_run(what, entry, kind, gtype, c, hp, _run(entry, kind, gtype, c, hp))


@pytest.mark.gpu
def test_misaligned_arrays_against_the_float64_oracle():
  """One array at a time 4 bytes off its 16-byte alignment: the 4-byte route of every row length that would otherwise
  move as 16-byte pieces."""
  routes = [('param', 'update'), ('grad', 'update'), ('grad', 'step'), ('m', 'update'), ('m', 'step'), ('v', 'update'),
            ('v', 'step'), ('out_step', 'step')]
  for d in D_MISALIGNED:
    for n, (which, entry) in enumerate(routes):
      kind = (d + n) % 2
      gtype = 'scalar' if which == 'v' or n % 2 else 'vector'          # (only the scalar groups' v is row-wise)
      c = _case(d * 31 + n, d, gtype)
      hp = _hp(bias_correction=bool(n % 3))
      _check_run(f"{entry} {which} misaligned d {d} {gtype}", entry, kind, gtype, c, hp,
                 _run(entry, kind, gtype, c, hp, misalign=(which,)))


def _group_c(gtype, t, d, hp):
  from taichi_splatting_amd import _lib
  g = _lib.OptimGroupC(group_type=oopt_group_type(gtype), param=_ptr(t['param']), grad=_ptr(t['grad']), m=_ptr(t['m']),
                       v=_ptr(t['v']), basis=_ptr(t.get('basis')), mask_lr=_ptr(t.get('mask')), point_lr=_ptr(t.get('plr')),
                       d=d, bias_correction=int(hp['bias_correction']), lr=hp['lr'], beta1=hp['betas'][0],
                       beta2=hp['betas'][1], eps=hp['eps'], clip=hp['clip'] if hp['clip'] is not None else -1.0, reserved=0.0)
  g.struct_size = ctypes.sizeof(_lib.OptimGroupC)
  return g


def _run_groups(kind, common, groups, hp, dense, misalign=()):
  """ms_optim_step_groups over groups [(gtype, arrays)] sharing `common`; dense: indexes NULL, weight -1 off the list.
  Returns (rc, [full-size GPU arrays per group])."""
  from taichi_splatting_amd import _lib
  lib = _lib.load()
  idx, n = common['idx'], common['tw'].shape[0]
  if dense:
    w = torch.full((n,), -1.0)
    w[idx] = common['w']
    gs = None
    if common['gs'] is not None:
      gs = torch.zeros(n)
      gs[idx] = common['gs']
    count, idx_g = n, None
  else:
    w, gs, count, idx_g = common['w'], common['gs'], idx.shape[0], _gpu(idx)
  w_g, tw_g, gs_g = _gpu(w), _gpu(common['tw']), _gpu(gs)
  ts, cs = [], []
  for gi, (gtype, a) in enumerate(groups):
    d = a['grad'].shape[1]
    t = {k: _gpu(a[k], (gi, k) in misalign) for k in ('param', 'grad', 'm', 'v')}
    if gtype == 'local_vector':
      b = a['basis']
      if dense:
        b = torch.zeros(n, d, d)
        b[idx] = a['basis']
      t['basis'] = _gpu(b)
    for k in ('mask', 'plr'):
      t[k] = _gpu(a.get(k))
    ts.append(t)
    cs.append(_group_c(gtype, t, d, hp))
  array = (_lib.OptimGroupC * len(cs))(*cs)
  rc = lib.ms_optim_step_groups(kind, array, len(cs), _ptr(idx_g), _ptr(w_g), _ptr(tw_g), _ptr(gs_g), count,
                                _lib.current_stream(torch.device(DEV)))
  torch.cuda.synchronize()
  return rc, ts


@pytest.mark.gpu
def test_all_row_lengths_in_one_step_groups_call_against_the_float64_oracle():
  """ms_optim_step_groups with every row length of the sweep as scalar and as vector groups plus two local_vector groups
  (fused groups flushed eight at a time, the rest launched on their own), with an index list and in the dense mode."""
  for kind in (0, 1):
    for bc in (True, False):
      for dense in (False, True):
        gen = torch.Generator().manual_seed(kind * 4 + bc * 2 + dense)
        common = _common(gen, 700, 300)
        common['gs'] = torch.rand(300, generator=gen) + 0.5
        hp = _hp(bias_correction=bc, clip=2.0)
        groups = [(gtype, _arrays(gen, 700, d, gtype, 300)) for d in D_SWEEP for gtype in ('scalar', 'vector')]
        groups += [('local_vector', _arrays(gen, 700, d, 'local_vector', 300)) for d in (2, 3)]
        rc, ts = _run_groups(kind, common, groups, hp, dense)
        _lib_check(rc, "ms_optim_step_groups")
        for (gtype, a), t in zip(groups, ts):
          c = dict(common, **a)
          _check_run(f"groups kind {kind} bc {bc} dense {dense} {gtype} d {a['grad'].shape[1]}", 'update', kind, gtype, c, hp,
                     dict(param=t['param'], m=t['m'], v=t['v']))


@pytest.mark.gpu
def test_edge_rows_against_the_float64_oracle():
  """Weights 0, 1e-3, 1, 50, 200 (beta^w underflows) with tw = w (a point's first step) and tw >> w, and tw = w = 0;
  betas (0, 0.5), (0.9, 0.999), (0.99, 0.9999); eps 1e-3, clip, mask_lr, point_lr and grad_scale binding; +inf, -inf
  and NaN gradient elements in scalar and vector rows: identical non-finite patterns in m, v and the raw step, and the
  parameters finite and within the error model."""
  for entry, kind, gtype, c, hp in _edge_cases():
    got = _run(entry, kind, gtype, c, hp)
    _check_run(f"edge {entry} kind {kind} {gtype} betas {hp['betas']} eps {hp['eps']}", entry, kind, gtype, c, hp, got)
    if entry == 'update':
      assert torch.isfinite(got['param']).all()


@pytest.mark.gpu
def test_fused_launch_is_bit_equal_to_one_launch_per_group():
  """Ten groups the fused kernel takes (two flushes of eight) and two it launches on their own (d = 27, local_vector) in
  one ms_optim_step_groups call, indexed and dense, against one ms_fractional_update per group.  Both instantiate
  update_point with the same arguments, and the results are the same bits except for the scalar groups moved as 16-byte
  pieces (d = 4, 16, 48): there the compiler contracts lerp's a t + b (1 - t) into a different fma at the two inline
  sites (a build with -ffp-contract=off makes every group bit-equal), so those are held to the float64 oracle's error
  model instead — both results."""
  fused = [('scalar', 1), ('scalar', 3), ('scalar', 4), ('scalar', 7), ('scalar', 16), ('scalar', 48), ('vector', 3),
           ('vector', 4), ('vector', 12), ('vector', 64)]
  assert all(_pick_shape(d) in ('S_V1_L1', 'S_V1_L4', 'S_V1_L16', 'S_V4_L1', 'S_V4_L4', 'S_V4_L16') for _, d in fused)
  for kind in (0, 1):
    for dense in (False, True):
      gen = torch.Generator().manual_seed(50 + kind * 2 + dense)
      common = _common(gen, 900, 500)
      common['gs'] = torch.rand(500, generator=gen) + 0.5
      hp = _hp(clip=1.0)
      groups = [(gtype, _arrays(gen, 900, d, gtype, 500)) for gtype, d in fused + [('scalar', 27), ('local_vector', 3)]]
      groups[2][1]['mask'] = torch.rand(4, generator=gen)
      groups[5][1]['plr'] = torch.rand(900, generator=gen) + 0.5
      rc, ts = _run_groups(kind, common, groups, hp, dense)
      _lib_check(rc, "ms_optim_step_groups")
      differ = []
      for gi, ((gtype, a), t) in enumerate(zip(groups, ts)):
        c = dict(common, **a)
        one = _run('update', kind, gtype, c, hp)
        if gtype == 'scalar' and _pick_shape(a['grad'].shape[1]).startswith('S_V4'):
          for run, got in (('fused', t), ('own launch', one)):
            _check_run(f"{run} kind {kind} dense {dense} group {gi}", 'update', kind, gtype, c, hp, got)
          continue
        for k in ('param', 'm', 'v'):
          if not torch.equal(t[k], one[k]):
            ulp = (t[k].view(torch.int32).long() - one[k].view(torch.int32).long()).abs().max()
            differ.append(f"group {gi} ({gtype}, d {a['grad'].shape[1]}) {k}: {int((t[k] != one[k]).sum())} elements, "
                          f"up to {int(ulp)} ulp")
      assert not differ, f"kind {kind} dense {dense}: not bit-equal: " + '; '.join(differ)


@pytest.mark.gpu
def test_fractional_step_writes_every_row_of_lr_step():
  """A negative weight on an index list is a weight (the skip sentinel belongs to the dense mode alone): every row of a
  NaN-filled lr_step is written, and moments and step follow the oracle (beta^w > 1)."""
  for kind in (0, 1):
    for gtype in ('scalar', 'vector'):
      c = _case(400 + kind * 2 + (gtype == 'vector'), 16, gtype)
      c['w'][::3] = -torch.rand(c['w'][::3].shape[0]) * 0.5 - 0.01
      c['m'] = c['m'] * 10 + 1.0                             # (no cancellation in lerp(beta^w > 1, v, g^2), which the
      c['v'] = c['v'] * 10 + 1.0                             # scale S_elem does not see: v >> g^2 |1 - beta^w|)
      got = _run('step', kind, gtype, c, _hp())
      assert not torch.isnan(got['step']).any(), f"kind {kind} {gtype}: rows of lr_step left unwritten"
      _check_run(f"negative weights step kind {kind} {gtype}", 'step', kind, gtype, c, _hp(), got)


@pytest.mark.gpu
def test_negative_weights_on_an_index_list_follow_the_oracle():
  for kind in (0, 1):
    for gtype, d in (('scalar', 5), ('vector', 48)):
      c = _case(500 + kind * 2 + (gtype == 'vector'), d, gtype)
      c['w'][1::2] = -torch.rand(c['w'][1::2].shape[0]) * 0.5 - 0.01
      c['m'] = c['m'] * 10 + 1.0
      c['v'] = c['v'] * 10 + 1.0
      hp = _hp()
      got = _run('update', kind, gtype, c, hp)
      _check_run(f"negative weights update kind {kind} {gtype}", 'update', kind, gtype, c, hp, got)


@pytest.mark.gpu
def test_step_groups_refuses_a_bad_group_before_any_launch():
  """[a valid group launched on its own (d = 100, misaligned), a valid fused group, an invalid group]: the error code,
  and every array bit for bit as before the call."""
  from taichi_splatting_amd import _lib
  gen = torch.Generator().manual_seed(9)
  common = _common(gen, 600, 300)
  groups = [('scalar', _arrays(gen, 600, 100, 'scalar')), ('vector', _arrays(gen, 600, 8, 'vector')),
            ('scalar', _arrays(gen, 600, 3, 'scalar'))]
  for bad, code in (('struct_size', MS_ERR_ABI), ('d', MS_ERR_BAD_ARG)):
    lib = _lib.load()
    idx_g, w_g, tw_g = _gpu(common['idx']), _gpu(common['w']), _gpu(common['tw'])
    ts = [{k: _gpu(a[k], gi == 0 and k == 'param') for k in ('param', 'grad', 'm', 'v')} for gi, (_, a) in enumerate(groups)]
    cs = [_group_c(gtype, t, a['grad'].shape[1], _hp()) for (gtype, a), t in zip(groups, ts)]
    if bad == 'struct_size':
      cs[2].struct_size -= 8
    else:
      cs[2].d = 0
    array = (_lib.OptimGroupC * 3)(*cs)
    rc = lib.ms_optim_step_groups(0, array, 3, _ptr(idx_g), _ptr(w_g), _ptr(tw_g), None, 300,
                                  _lib.current_stream(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == code, f"bad {bad}: rc {rc}, expected {code}"
    for gi, ((_, a), t) in enumerate(zip(groups, ts)):
      for k in ('param', 'm', 'v'):
        assert torch.equal(t[k].cpu(), a[k]), f"bad {bad}: group {gi} {k} changed by a refused call"
