"""The scenes and the float64 truth of tests/autograd_cases.py, checked on the CPU with the oracle alone.

These are conditions on the INPUTS of tests/test_gpu_autograd_contract.py, not measurements of the kernels: enough rows
culled (and none on the second scene), no SH colour on the edge of its clamp, gate-stable splats, a float32 oracle that
culls the same rows — and the autograd node the truth is built on (oracle.raster.forward / backward) agreeing with the
differentiable restatement (oracle.raster.rasterize_autograd) and with the pipeline tests/test_gpu_render.py assembles."""
import pytest
import torch

from oracle import raster as orast
from . import autograd_cases as ac


def test_culled_share_of_both_scenes():
  share = ac.culled_rows('culled').double().mean().item()
  assert 0.10 <= share <= 0.60, share
  assert int(ac.culled_rows('all').sum()) == 0
  for kind in ac.SCENES:
    g, camera = ac.scene(kind)
    assert g.position.shape == (ac.N, 3) and camera.image_size == ac.SIZE
    for t in (g.position, g.log_scaling, g.rotation, g.alpha_logit, g.feature, camera.T_camera_world, camera.projection):
      assert torch.equal(t, t.float().double())                # float32-representable: one set of values for both dtypes


@pytest.mark.parametrize('kind', list(ac.SCENES))
def test_sh_colours_stay_off_the_clamp_edges(kind):
  assert ac.sh_clamp_margin(kind) > 1e-5
  out, _ = ac.sh_truth(kind, 'unique')
  assert 0 < int(((out <= 0) | (out >= 1)).sum()) < out.numel() // 2       # the clamp is reached, by a minority


@pytest.mark.parametrize('kind', list(ac.SCENES))
def test_scenes_are_gate_stable(kind):
  assert ac.geometry(kind)[2] >= 0.70                           # share of the pool's splats that survived
  for antialias in (False, True):
    cfg = ac.config(antialias=antialias)
    for features in ('rgb', 'sh3'):
      want = ac.frame_truth(kind, features, 'weighted', antialias)
      assert float(orast.gate_margin(want.gaussians2d, want.ranges, want.o2p, ac.SIZE, cfg).min()) > ac.GATE_MARGIN
  x = ac.raster_inputs(kind, 'rgb')                             # the splats rounded to float32 as well
  assert float(orast.gate_margin(x.gaussians2d, x.ranges, x.o2p, ac.SIZE, ac.config()).min()) > 0.5 * ac.GATE_MARGIN


@pytest.mark.parametrize('kind', list(ac.SCENES))
def test_float32_oracle_culls_the_same_rows(kind):
  """the yardstick of the float32 projection backward: the oracle's chain in float32 on the float64 truth's own upstream
  gradients keeps the rows, reproduces the truth in float64 and the well-conditioned leaves in float32"""
  want = ac.frame_truth(kind, 'sh3', 'mixed')
  w64, w32 = ac.chain_grads(kind, 'sh3', torch.float64, want.upstream), ac.chain_grads(kind, 'sh3', torch.float32, want.upstream)
  for name in ac.ALL_LEAVES:
    truth = want.grads[name]
    assert float(truth.abs().max()) > 0, name
    assert (w64[name] - truth).abs().max().item() <= 1e-12 * truth.abs().max().item(), name
  for name in ('alpha_logit', 'feature'):
    assert (w32[name] - w64[name]).abs().max().item() <= 1e-4 * w64[name].abs().max().item(), name
  assert torch.equal(ac.projection_truth(kind, 'both', torch.float32)[2], ac.projection_truth(kind, 'both')[2])


@pytest.mark.parametrize('features', ['rgb', 'sh3'])
def test_truth_is_the_pipeline_of_test_gpu_render(features):
  from .test_gpu_render import oracle_render_with_grads
  g, camera = ac.scene('culled', features)
  cfg = ac.config()
  want = ac.frame_truth('culled', features, 'weighted')
  image, alpha, idx, grads = oracle_render_with_grads(g, camera, cfg, features == 'sh3', ac.constants(3).G)
  assert torch.equal(idx, want.idx)
  assert torch.allclose(image, want.image, rtol=0, atol=1e-13) and torch.allclose(alpha, want.image_weight, rtol=0, atol=1e-13)
  for name, theirs in zip(ac.LEAVES, grads):
    assert torch.allclose(theirs, want.grads[name], rtol=1e-12, atol=1e-12 * float(theirs.abs().max())), name


@pytest.mark.parametrize('kind', list(ac.SCENES))
@pytest.mark.parametrize('antialias', [False, True])
def test_raster_node_is_the_differentiable_restatement(kind, antialias):
  """oracle.raster.backward drops the pairs behind a pixel's saturation point, rasterize_autograd does not: no pair of
  these scenes lies behind one, so the two are one function here."""
  x = ac.raster_inputs(kind, 'rgb')
  cfg = ac.config(antialias=antialias)
  want = ac.raster_truth(kind, 'rgb', 'weighted', antialias)
  margin, side = orast.saturation_margin(x.gaussians2d, x.ranges, x.o2p, ac.SIZE, cfg)
  assert int((side < 0).sum()) == 0 and float(margin.min()) > 1e-3        # no pair dropped, none near the test
  p, f = x.gaussians2d.clone().requires_grad_(True), x.features.clone().requires_grad_(True)
  image = orast.rasterize_autograd(p, f, x.ranges, x.o2p, ac.SIZE, cfg)
  assert torch.allclose(image, want.image, atol=1e-12)
  (image * ac.constants(3).G).sum().backward()
  for got, name in ((p.grad, 'gaussians2d'), (f.grad, 'features')):
    ref = want.grads[name]
    assert (got - ref).abs().max().item() <= 1e-10 * max(1.0, ref.abs().max().item()), name


def test_truth_has_the_properties_the_checks_lean_on():
  for features in ('rgb', 'c4', 'sh3'):
    whole = ac.frame_truth('culled', features, 'weighted')
    a, b = ac.frame_truth('culled', features, 'half_a'), ac.frame_truth('culled', features, 'half_b')
    culled = ac.culled_rows('culled')
    for name in ac.ALL_LEAVES:
      w = whole.grads[name]
      assert float(w.abs().max()) > 0, (features, name)
      assert (a.grads[name] + b.grads[name] - w).abs().max().item() <= 1e-12 * w.abs().max().item(), (features, name)
      if name in ac.LEAVES:
        assert float(w[culled].abs().max()) == 0.0 and float(w[~culled].abs().max()) > 0
    assert float(whole.heuristic[culled].abs().max()) == 0.0 and float(whole.heuristic.abs().max()) > 0
    assert float(whole.visibility[~culled].min()) >= 0 and float(whole.visibility.max()) > 0
  # an expanded scalar and its materialised form are one loss
  s, o = ac.frame_truth('culled', 'rgb', 'sum'), ac.frame_truth('culled', 'rgb', 'ones')
  for name in ac.ALL_LEAVES:
    assert torch.equal(s.grads[name], o.grads[name]), name
  # the losses on points alone reach the leaves they should, and only those
  d = ac.frame_truth('culled', 'sh3', 'depths').grads
  assert float(d['position'].abs().max()) > 0 and float(d['feature'].abs().max()) == 0 and float(d['alpha_logit'].abs().max()) == 0
  f = ac.frame_truth('culled', 'sh3', 'features').grads
  assert float(f['feature'].abs().max()) > 0 and float(f['log_scaling'].abs().max()) == 0
  assert float(f['T_camera_world'].abs().max()) > 0            # the SH direction sees the camera position


def test_subsets_are_singles_and_all_but_one():
  assert ac.subsets(ac.RASTER_LEAVES) == [('gaussians2d',), ('features',)]
  got = ac.subsets(ac.ALL_LEAVES)
  assert len(got) == 14 and all(len(s) in (1, 6) for s in got) and len(set(got)) == 14
