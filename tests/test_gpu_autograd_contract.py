"""-m gpu: the autograd contract of the five ``torch.autograd.Function`` wrappers (projection, SH, rasterize_with_tiles,
rasterize, the frame) and of the loss on top of them — what the C-ABI tests cannot see: which gradient buffers are
``torch.empty`` and which ``torch.zeros``, which pointers are NULL, what ``None`` / expanded / non-contiguous upstream
gradients become, and what a second backward over one graph does.

Truth is float64 torch autograd through the oracle pipeline on the same input values (tests/autograd_cases.py, whose
scenes tests/test_autograd_cases_host.py checks on the CPU).  Tolerances are the project's own: float64 1e-9 on images
and the gradient tolerances of tests/test_gpu_raster.py::test_forward_backward_f64; float32 1e-4 of the largest value
(``assert_within``) — the frame executor's fused backward included, on every leaf —, except the leaves behind the MODULAR
float32 projection backward (``projection.apply`` and the legacy ``render_gaussians``: position, log_scaling, rotation,
camera), ill-conditioned on a few rows by design, which are held to
tests/test_gpu_projection_sh.py::assert_f32_gradient_as_accurate_as_reference: against the oracle's chain in float64 and in
float32 on the gradients that backward was handed (for the legacy render: the raster kernel's own 2D gradients).

A  subsets of ``requires_grad``: every single leaf and all-but-one, allocator poisoned with NaN before each backward;
B  ``backward(retain_graph=True)`` three times as bench.py times it, and two frames of one shape interleaved;
C  a loss split over two backward passes into a preset ``.grad``, then an unrelated frame that must not touch it;
D  upstream forms: ``None`` for the image, expanded scalar, non-contiguous, one output of two;
E  point heuristics: every backward pass leaves the heuristics OF THAT PASS (INTEGRATION.md difference 19).  Before this
   file the generic kernels (float64, 4 or 9 channels, antialias) added into the tensor the forward had zeroed once, so
   a second pass over one graph doubled them while the float32 RGB moments path stored: on that parent the generic cases
   of ``test_heuristics_are_those_of_the_last_pass`` fail with a factor of 2 at pass 2 and 3 at pass 3.

Where a path has no float atomics the subset / repeated results are compared with ``torch.equal``: the projection's
per-row outputs, SH on unique indexes, and — with ``rasterizer.function.DETERMINISTIC_BACKWARD`` on — everything
behind the float32 RGB raster backward except the camera sums (subsets of the legacy render of an SH scene excepted:
their forward differs in the last bit with the pose's ``requires_grad``).  Elsewhere: ``assert_grads_close`` of
tests/test_gpu_frame.py.

Every case is 300 gaussians on 64 x 48 and the oracle results are cached per (scene, features, loss): the 251 cases take
about 8 s on an MI355X, the slowest (a subset matrix of fifteen forward + backward runs) about 1 s."""
import types
from dataclasses import replace

import pytest
import torch

from taichi_splatting_amd import Gaussians3D, evaluate_sh_at, frame, rasterize, rasterize_with_tiles, render_gaussians
from taichi_splatting_amd.loss import l1_ssim_loss
from taichi_splatting_amd.perspective import projection as hip_projection
from taichi_splatting_amd.rasterizer import function as raster_function
from . import autograd_cases as ac
from .test_gpu_raster import assert_within

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
DTYPES = pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])


@pytest.fixture(autouse=True)
def deterministic(monkeypatch):
  """fixed-point commits on the float32 RGB raster backward (tests that want the float atomics switch it off again)"""
  monkeypatch.setattr(raster_function, 'DETERMINISTIC_BACKWARD', True)


# ---- the operators, behind one surface ----------------------------------------------------------------------------------------

class Op:
  """leaves: names of the differentiable inputs; fresh(requires) -> dict of new leaf tensors on the GPU; forward(leaves)
  -> out; loss(out, name) -> scalar; want(name) -> truth namespace with .grads; zero_rows(leaf) -> rows that must be
  exactly zero; exact: leaves whose gradient involves no float atomic; losses: (whole, half a, half b)."""
  losses = ('weighted', 'half_a', 'half_b')
  moments = False

  def __init__(self, kind, features, dtype, **cfg):
    self.kind, self.features, self.dtype, self.cfg = kind, features, dtype, ac.config(**cfg)
    self.antialias = bool(cfg.get('antialias', False))
    self.moments = dtype == F32 and features in ('rgb', 'sh3') and not self.antialias       # the float32 RGB product path

  def __repr__(self):
    return f"{type(self).__name__}({self.kind}, {self.features}, {self.dtype}, {getattr(self, 'path', '')})"

  def references(self, name, out):
    """(w64, w32) of assert_f32_gradient_as_accurate_as_reference for the leaves that criterion applies to, or (None, None)"""
    return None, None

  def reset(self, out):
    """forget what an earlier backward pass accumulated outside the leaves"""

  def zero_rows(self, leaf):
    return None

  def other(self):
    """the same operator on the other scene (same shapes)"""
    twin = object.__new__(type(self))
    twin.__dict__.update(self.__dict__)
    twin.kind = 'all' if self.kind == 'culled' else 'culled'
    return twin


class RenderOut:
  """the differentiable outputs of a Rendering; ``points`` are touched (and compacted) only by a loss that reads them"""

  def __init__(self, rendering):
    self.r = rendering
  image = property(lambda s: s.r.image)
  image_weight = property(lambda s: s.r.image_weight)
  gaussians2d = property(lambda s: s.r.points.gaussians2d)
  depths = property(lambda s: s.r.points.depths)
  features = property(lambda s: s.r.points.features)
  idx = property(lambda s: s.r.points.idx)


class RenderOp(Op):
  leaves = ac.ALL_LEAVES

  def __init__(self, path, kind, features, dtype, **cfg):
    super().__init__(kind, features, dtype, **cfg)
    self.path = path

  @property
  def exact(self):
    return ac.LEAVES if self.moments and raster_function.DETERMINISTIC_BACKWARD else ()

  @property
  def exact_across_subsets(self):
    # the modular path takes the camera position of an SH scene from torch.inverse when the pose requires grad and from its
    # own kernel otherwise (last-bit differences, tests/test_gpu_frame.py): two subsets then differ in their FORWARD
    return () if self.path == 'legacy' and self.features == 'sh3' else self.exact

  def fresh(self, requires):
    return ac.scene_leaves(self.kind, self.features, self.dtype, DEV, requires)

  def forward(self, leaves):
    camera = ac.scene(self.kind, self.features, self.dtype)[1].to(device=DEV)
    camera = replace(camera, T_camera_world=leaves['T_camera_world'], projection=leaves['projection'])
    g = Gaussians3D(**{name: leaves[name] for name in ac.LEAVES}, batch_size=(ac.N,))
    before, frame.USE_FRAME = frame.USE_FRAME, self.path == 'frame'
    try:
      r = render_gaussians(g, camera, self.cfg, use_sh=self.features == 'sh3')
    finally:
      frame.USE_FRAME = before
    assert hasattr(r, 'frame') == (self.path == 'frame' and ac.FEATURES[self.features] <= 4)
    out = RenderOut(r)
    # the frame's full-size outputs, taken before ``points`` is compacted (which hands out copies of the rows in view)
    out.full_size = frame.point_outputs(r) if hasattr(r, 'frame') else None
    out.boundary = None
    if self.path == 'legacy' and self.dtype == F32:
      # what the modular projection (and SH) backward will be handed: its yardstick is evaluated on these (references)
      out.boundary = [r.points.gaussians2d, r.points.depths, r.points.features if self.features == 'sh3' else None]
      for t in out.boundary:
        if t is not None and t.requires_grad:
          t.retain_grad()
    return out

  def loss(self, out, name):
    if name == 'photometric':
      return l1_ssim_loss(out.image, ac.constants(3, self.dtype, DEV).target)
    return ac.LOSSES[name](out)

  def want(self, name):
    return ac.frame_truth(self.kind, self.features, name, self.antialias)

  def references(self, name, out):
    if out is None or out.boundary is None:
      return None, None
    upstream = [None if t is None else t.grad for t in out.boundary]
    w64, w32 = (ac.chain_grads(self.kind, self.features, dtype, upstream) for dtype in (F64, F32))
    keep = lambda w: {leaf: w[leaf] for leaf in ac.ILL_CONDITIONED_F32}
    return keep(w64), keep(w32)

  def reset(self, out):
    for t in out.boundary or ():
      if t is not None:
        t.grad = None

  def zero_rows(self, leaf):
    return ac.culled_rows(self.kind) if leaf in ac.LEAVES else None

  def point_outputs(self, out):
    """(visibility (N,) or None, heuristics (N, 2) or None) at full size, read NOW (not a copy made earlier)"""
    r = out.r
    if out.full_size is not None:
      return out.full_size['visibility'], out.full_size['point_heuristic']
    idx, cfg = r.points.idx, self.cfg
    vis = heur = None
    if cfg.compute_visibility:
      vis = torch.zeros(ac.N, dtype=self.dtype, device=DEV).index_copy_(0, idx, r.points.visibility)
    if cfg.compute_point_heuristic:
      heur = torch.zeros(ac.N, 2, dtype=self.dtype, device=DEV)
      heur[idx] = torch.stack([r.points.prune_cost, r.points.split_score], dim=1)
    return vis, heur


class RasterOp(Op):
  leaves = ac.RASTER_LEAVES

  def __init__(self, path, kind, features, dtype, **cfg):
    super().__init__(kind, features, dtype, **cfg)
    self.path = path

  @property
  def exact(self):
    return ac.RASTER_LEAVES if self.moments and raster_function.DETERMINISTIC_BACKWARD else ()

  def fresh(self, requires):
    x = ac.raster_inputs(self.kind, self.features)
    return {name: getattr(x, name).to(self.dtype).to(DEV).requires_grad_(name in requires) for name in self.leaves}

  def forward(self, leaves):
    x = ac.raster_inputs(self.kind, self.features)
    if self.path == 'tiles':
      out = rasterize_with_tiles(leaves['gaussians2d'], leaves['features'], x.o2p.to(DEV), x.ranges.to(DEV), ac.SIZE, self.cfg)
    else:
      out = rasterize(leaves['gaussians2d'], x.depth.to(self.dtype).to(DEV), leaves['features'], ac.SIZE, self.cfg)
    return out

  def loss(self, out, name):
    return ac.LOSSES[name](out)

  def want(self, name):
    return ac.raster_truth(self.kind, self.features, name, self.antialias)

  def point_outputs(self, out):
    return (out.visibility if self.cfg.compute_visibility else None,
            out.point_heuristic if self.cfg.compute_point_heuristic else None)


class ProjectionOp(Op):
  leaves = ac.PROJECTION_LEAVES
  exact = ac.LEAVES[:4]                        # per-row outputs: plain stores; the camera sums are atomics
  losses = ('both', 'points', 'depth')

  def fresh(self, requires):
    leaves = ac.scene_leaves(self.kind, 'rgb', self.dtype, DEV, requires)
    return {name: leaves[name] for name in self.leaves}

  def forward(self, leaves):
    camera, cfg = ac.scene(self.kind)[1], self.cfg
    points, depth, idx = hip_projection.apply(*[leaves[name] for name in self.leaves], ac.SIZE, camera.depth_range,
                                              cfg.blur_cov, cfg.clamp_margin, cfg.alpha_threshold)
    return types.SimpleNamespace(points=points, depth=depth, idx=idx)

  def loss(self, out, name):
    return ac.projection_loss(out.points, out.depth, out.idx, name)

  def want(self, name):
    points, depth, idx, grads = ac.projection_truth(self.kind, name)
    return types.SimpleNamespace(points=points, depth=depth, idx=idx, grads=grads)

  def references(self, name, out):
    return (None, None) if self.dtype == F64 else (None, ac.projection_truth(self.kind, name, F32)[3])

  def zero_rows(self, leaf):
    return ac.culled_rows(self.kind) if leaf in ac.LEAVES else None


class ShOp(Op):
  leaves = ac.SH_LEAVES

  def __init__(self, which, kind, dtype):
    super().__init__(kind, 'sh3', dtype)
    self.which = self.path = which

  @property
  def exact(self):
    return ('feature', 'position') if self.which == 'unique' else ()      # one plain store / one add per row

  def fresh(self, requires):
    g = ac.scene(self.kind, 'sh3', self.dtype)[0]
    values = dict(feature=g.feature, position=g.position, camera_position=ac.sh_camera_position(self.kind).to(self.dtype))
    return {name: t.detach().clone().to(DEV).requires_grad_(name in requires) for name, t in values.items()}

  def forward(self, leaves):
    idx = ac.sh_indexes(self.kind, self.which).to(DEV)
    return evaluate_sh_at(leaves['feature'], leaves['position'], idx, leaves['camera_position'],
                          unique_indexes=self.which == 'unique')

  def loss(self, out, name):
    return ac.sh_loss(out, name)

  def want(self, name):
    out, grads = ac.sh_truth(self.kind, self.which, name)
    return types.SimpleNamespace(out=out, grads=grads)

  def zero_rows(self, leaf):
    if leaf == 'camera_position':
      return None
    untouched = torch.ones(ac.N, dtype=torch.bool)
    untouched[ac.sh_indexes(self.kind, self.which)] = False
    return untouched


def render_ops(features=('rgb', 'c4', 'sh3'), kinds=('culled', 'all'), dtypes=(F32, F64), **cfg):
  return [RenderOp(path, kind, f, dtype, **cfg) for path in ('frame', 'legacy') for kind in kinds for f in features
          for dtype in dtypes]


def raster_ops(features=('rgb', 'c4'), kinds=('culled',), dtypes=(F32, F64), **cfg):
  return [RasterOp(path, kind, f, dtype, **cfg) for path in ('tiles', 'rasterize') for kind in kinds for f in features
          for dtype in dtypes]


def modular_ops():
  return ([ProjectionOp(kind, 'rgb', dtype) for kind in ('culled', 'all') for dtype in (F32, F64)]
          + [ShOp(which, kind, dtype) for which in ('unique', 'repeated') for kind in ('culled', 'all') for dtype in (F32, F64)])


def op_id(op):
  dtype = 'f32' if op.dtype == F32 else 'f64'
  return f"{type(op).__name__}-{getattr(op, 'path', '')}-{op.kind}-{op.features}-{dtype}" + ('-aa' if op.antialias else '')


EVERY_OP = render_ops() + raster_ops(kinds=('culled', 'all')) + modular_ops()


# ---- shared steps ----------------------------------------------------------------------------------------------------------------

def check_against_truth(op, leaves, names, loss, what, grads=None, out=None):
  """finite, exactly zero where no gradient can arrive, equal to the float64 oracle's"""
  want = op.want(loss)
  w64, w32 = op.references(loss, out)
  for name in names:
    got = leaves[name].grad if grads is None else grads[name]
    if got is None:
      # no path from the loss to this leaf through the modular graph: autograd never calls a backward for it
      assert float(want.grads[name].abs().max()) == 0.0, (what, name, 'no gradient')
      continue
    assert bool(torch.isfinite(got).all()), (what, name, 'not finite')
    rows = op.zero_rows(name)
    if rows is not None and bool(rows.any()):
      assert float(got[rows.to(DEV)].abs().max()) == 0.0, (what, name, 'rows without a gradient are not exactly zero')
    ac.assert_gradient(name, got, want.grads[name], op.dtype, what, w32, w64)


def backward_all_leaves(op, loss):
  leaves = op.fresh(op.leaves)
  out = op.forward(leaves)
  ac.poison(*leaves.values())
  op.loss(out, loss).backward()
  return leaves, out


def check_forward(op, out):
  """the forward quantities against the oracle's, once per operator (1e-9 float64, 1e-4 float32)"""
  tol = 1e-9 if op.dtype == F64 else 1e-4
  want = op.want(op.losses[0])
  if isinstance(op, ProjectionOp):
    assert torch.equal(out.idx.cpu(), want.idx)
    if op.dtype == F64:
      assert torch.allclose(out.points.detach().cpu(), want.points) and torch.allclose(out.depth.detach().cpu(), want.depth)
  elif isinstance(op, ShOp):
    assert (out.detach().cpu().double() - want.out).abs().max().item() <= (1e-12 if op.dtype == F64 else 1e-5)
  else:
    assert (out.image.detach().cpu().double() - want.image).abs().max().item() < tol
    assert (out.image_weight.detach().cpu().double() - want.image_weight).abs().max().item() < tol
    if isinstance(op, RenderOp):
      assert torch.equal(out.idx.cpu(), want.idx)


# ---- A: subsets of requires_grad -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('op', EVERY_OP, ids=op_id)
def test_subsets_of_requires_grad(op):
  loss = op.losses[0]
  full, out = backward_all_leaves(op, loss)
  check_forward(op, out)
  check_against_truth(op, full, op.leaves, loss, (op, 'all leaves'), out=out)
  full = {name: t.grad.clone() for name, t in full.items()}
  for subset in ac.subsets(op.leaves):
    leaves = op.fresh(subset)
    out = op.forward(leaves)
    ac.poison(*[leaves[name] for name in subset])
    op.loss(out, loss).backward()
    what = (op, subset)
    for name in op.leaves:
      if name not in subset:
        assert leaves[name].grad is None, (what, name, 'a gradient for a leaf that asked for none')
    check_against_truth(op, leaves, subset, loss, what, out=out)
    for name in subset:
      ac.assert_same_gradient(name, leaves[name].grad, full[name], op.dtype, name in getattr(op, 'exact_across_subsets', op.exact), what)


# ---- B: repeated backward ---------------------------------------------------------------------------------------------------------

def point_output_checks(op, out, what, heuristics_too=True):
  """visibility is a forward quantity: the oracle's after every pass.  Heuristics: the oracle's of ONE pass (E)."""
  if not hasattr(op, 'point_outputs'):
    return
  vis, heur = op.point_outputs(out)
  want = op.want(op.losses[0])
  if vis is not None:
    if op.dtype == F64:
      assert torch.allclose(vis.cpu(), want.visibility, atol=1e-8), (what, 'visibility')
    else:
      assert_within(vis, want.visibility, 1e-4, (what, 'visibility'))
  if heur is not None and heuristics_too:
    check_heuristics(op, heur, want.heuristic, what)


def check_heuristics(op, got, want, what):
  """tests/test_gpu_raster.py::test_point_heuristics_with_wide_features: 1e-8 (float64) / 1e-4 (float32) of max(1, largest)"""
  tol = 1e-8 if op.dtype == F64 else 1e-4
  scale = max(1.0, want.abs().max().item())
  err = (got.cpu().double() - want).abs().max().item()
  ratio = (got.cpu().double().abs().sum() / want.abs().sum()).item()
  print(f"{what}: heuristics max err {err:.3e}, scale {scale:.3e}, sum(got) / sum(want) {ratio:.4f}")
  assert err < tol * scale, (what, 'heuristics', err, scale, f"sum ratio {ratio:.4f}")


def repeated_backward(op, loss, passes=3):
  leaves = op.fresh(op.leaves)
  out = op.forward(leaves)
  value = op.loss(out, loss)
  seen = []
  for k in range(passes):
    for t in leaves.values():
      t.grad = None               # as bench.py does between its timed passes
    op.reset(out)
    ac.poison(*leaves.values())
    value.backward(retain_graph=True)
    check_against_truth(op, leaves, op.leaves, loss, (op, loss, f'pass {k + 1}'), out=out)
    point_output_checks(op, out, (op, loss, f'pass {k + 1}'))
    seen.append({name: t.grad.clone() for name, t in leaves.items()})
  for k in range(1, passes):
    for name in op.exact:
      assert torch.equal(seen[k][name], seen[0][name]), (op, name, f'pass {k + 1} is not pass 1 bit for bit')


REPEATED = ([RenderOp(path, 'culled', f, dtype, heuristic=flags, visibility=flags)
             for path in ('frame', 'legacy') for f, dtype in (('rgb', F32), ('sh3', F32), ('rgb', F64), ('c4', F32))
             for flags in (False, True)]
            + raster_ops(heuristic=True, visibility=True) + modular_ops())


@pytest.mark.parametrize('op', REPEATED, ids=lambda op: op_id(op) + ('-outputs' if op.cfg.compute_visibility else ''))
def test_three_backward_passes_over_one_graph(op):
  repeated_backward(op, op.losses[0])


@pytest.mark.parametrize('op', [RenderOp('frame', 'culled', 'rgb', F32, heuristic=True, visibility=True),
                                RasterOp('tiles', 'culled', 'rgb', F32, heuristic=True)], ids=op_id)
def test_three_backward_passes_with_float_atomics(op, monkeypatch):
  """the default backward (float atomic commits into the shared accumulator): every pass within tolerance"""
  monkeypatch.setattr(raster_function, 'DETERMINISTIC_BACKWARD', False)
  assert op.exact == ()
  repeated_backward(op, op.losses[0])


def test_three_backward_passes_with_visibility_from_the_backward(monkeypatch):
  """``frame.VISIBILITY_FROM_BACKWARD``: the forward defers the visibility, a read before the backward computes it on
  demand and every backward pass STORES it again (column 11 of the moment rows) — the sum over the pairs the backward
  visits, which on these scenes is every pair (tests/test_autograd_cases_host.py: none lies behind a saturation point),
  so it stays the oracle's forward visibility after each pass."""
  monkeypatch.setattr(frame, 'VISIBILITY_FROM_BACKWARD', True)
  op = RenderOp('frame', 'culled', 'rgb', F32, heuristic=True, visibility=True)
  before = frame.visibility_passes
  repeated_backward(op, 'weighted')
  assert frame.visibility_passes == before + 1               # deferred indeed, and computed on demand once


@pytest.mark.parametrize('path', ['frame', 'legacy'])
@DTYPES
def test_three_backward_passes_through_the_photometric_loss(path, dtype):
  """render -> l1_ssim_loss -> backward(retain_graph=True) x 3: the loss node is differentiable once per pass, any number
  of passes; truth is tests/photometric_oracle.py::loss_terms on the oracle's image"""
  repeated_backward(RenderOp(path, 'culled', 'rgb', dtype), 'photometric')


@pytest.mark.parametrize('features,dtype', [('rgb', F32), ('rgb', F64), ('c4', F32)], ids=['moments', 'f64', 'c4'])
@pytest.mark.parametrize('path', ['frame', 'legacy'])
def test_two_frames_of_one_shape_interleaved(path, features, dtype):
  """forward A, forward B, backward A, backward B, backward A again: the frames share the per-device moments accumulator
  (and the scene shape's record); no pass may see the other frame's sums"""
  a = RenderOp(path, 'culled', features, dtype, heuristic=True, visibility=True)
  b = a.other()
  la, lb = a.fresh(a.leaves), b.fresh(b.leaves)
  oa, ob = a.forward(la), b.forward(lb)
  va, vb = a.loss(oa, 'weighted'), b.loss(ob, 'weighted')
  first = None
  for k, (op, leaves, out, value) in enumerate(((a, la, oa, va), (b, lb, ob, vb), (a, la, oa, va))):
    for t in leaves.values():
      t.grad = None
    op.reset(out)
    ac.poison(*leaves.values())
    value.backward(retain_graph=True)
    check_against_truth(op, leaves, op.leaves, 'weighted', (op, f'interleaved step {k}'), out=out)
    point_output_checks(op, out, (op, f'interleaved step {k}'))
    if k == 0:
      first = {name: t.grad.clone() for name, t in leaves.items()}
  for name in a.exact:
    assert torch.equal(la[name].grad, first[name]), (a, name, 'the second backward of frame A saw frame B')


# ---- C: a loss split over two passes, into a preset .grad ----------------------------------------------------------------------

@pytest.mark.parametrize('op', render_ops(kinds=('culled',)) + raster_ops() + modular_ops(), ids=op_id)
def test_split_loss_accumulates_into_a_preset_grad(op):
  whole, half_a, half_b = op.losses
  want = op.want(whole)
  leaves = op.fresh(op.leaves)
  gen = torch.Generator().manual_seed(41)
  preset = {}
  for name, t in leaves.items():
    # of the gradient's own size, so that the sum keeps the gradient's digits
    scale = max(want.grads[name].abs().max().item(), 1e-30)
    preset[name] = (scale * torch.rand(t.shape, generator=gen, dtype=torch.float64)).to(op.dtype).to(DEV)
    t.grad = preset[name].clone()
  out = op.forward(leaves)
  ac.poison(*leaves.values())
  op.loss(out, half_a).backward(retain_graph=True)
  ac.poison(*leaves.values())
  op.loss(out, half_b).backward()
  added = {name: t.grad - preset[name] for name, t in leaves.items()}
  check_against_truth(op, leaves, op.leaves, whole, (op, 'split loss'), grads=added, out=out)
  # a returned gradient must not alias a buffer that a later frame writes
  kept = {name: t.grad.clone() for name, t in leaves.items()}
  backward_all_leaves(op.other(), whole)
  torch.cuda.synchronize()
  for name, t in leaves.items():
    assert torch.equal(t.grad, kept[name]), (op, name, 'changed by an unrelated frame')


# ---- D: upstream forms -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('upstream', ['depth', 'points'])
@pytest.mark.parametrize('kind', ['culled', 'all'])
@DTYPES
def test_projection_with_one_upstream_gradient(kind, dtype, upstream):
  op = ProjectionOp(kind, 'rgb', dtype)
  leaves, out = backward_all_leaves(op, upstream)
  check_against_truth(op, leaves, op.leaves, upstream, (op, upstream), out=out)


@pytest.mark.parametrize('loss', ['depths', 'gaussians2d', 'features', 'mixed'])
@pytest.mark.parametrize('op', render_ops(features=('rgb', 'sh3'), kinds=('culled',)), ids=op_id)
def test_render_differentiated_through_points(op, loss):
  """``g_image is None`` (or, 'mixed', everything at once): the loss reads ``rendering.points`` only"""
  leaves, out = backward_all_leaves(op, loss)
  check_against_truth(op, leaves, op.leaves, loss, (op, loss), out=out)


@pytest.mark.parametrize('loss', ['sum', 'permuted', 'strided'])
@pytest.mark.parametrize('op', render_ops(features=('rgb', 'c4'), kinds=('culled',)) + raster_ops(), ids=op_id)
def test_unusual_image_gradients(op, loss):
  """an expanded scalar (``image.sum()``), a non-contiguous dL/dimage (a channel of ``image.permute(2, 0, 1)``) and a
  strided slice, all against the oracle; the expanded scalar also against the same loss written as (image * ones).sum()"""
  leaves, out = backward_all_leaves(op, loss)
  check_against_truth(op, leaves, op.leaves, loss, (op, loss), out=out)
  if loss == 'sum':
    ones, _ = backward_all_leaves(op, 'ones')
    for name in op.leaves:
      ac.assert_same_gradient(name, leaves[name].grad, ones[name].grad, op.dtype, False, (op, 'sum vs ones'))


@pytest.mark.parametrize('op', render_ops(features=('rgb',), kinds=('culled',), heuristic=True, visibility=True)
                         + raster_ops(features=('rgb',), heuristic=True, visibility=True), ids=op_id)
def test_non_differentiable_outputs_start_no_backward(op):
  """image_weight, visibility and the heuristics carry no graph: a loss on them alone cannot be differentiated, and
  added to a real loss they change nothing and receive no kernel launch of their own"""
  leaves = op.fresh(op.leaves)
  out = op.forward(leaves)
  vis, heur = op.point_outputs(out)
  for t in (out.image_weight, vis, heur):
    assert not t.requires_grad and t.grad_fn is None
  with pytest.raises(RuntimeError):
    out.image_weight.sum().backward()
  assert all(t.grad is None for t in leaves.values())
  (op.loss(out, 'weighted') + 3.0 * out.image_weight.sum() + vis.sum()).backward()
  check_against_truth(op, leaves, op.leaves, 'weighted', (op, 'image + image_weight'), out=out)


# ---- E: the heuristics of the last pass ---------------------------------------------------------------------------------------

HEURISTIC_OPS = ([RenderOp(path, 'culled', f, dtype, heuristic=True, antialias=aa)
                  for path in ('frame', 'legacy')
                  for f, dtype, aa in (('rgb', F32, False), ('c4', F32, False), ('rgb', F64, False), ('rgb', F32, True), ('c9', F32, False))]
                 + [RasterOp(path, 'culled', f, dtype, heuristic=True, antialias=aa)
                    for path in ('tiles', 'rasterize')
                    for f, dtype, aa in (('rgb', F32, False), ('c4', F32, False), ('rgb', F64, False), ('rgb', F32, True), ('c9', F32, False),
                                         ('c9', F64, False))])


@pytest.mark.parametrize('op', HEURISTIC_OPS, ids=op_id)
def test_heuristics_are_those_of_the_last_pass(op):
  """prune_cost / split_score after one, two and three backward passes over one graph: the oracle's of a SINGLE pass, on the
  float32 RGB moments path (which always stored) and on the generic kernels (float64, 4 and 9 channels — the zero-padded
  wide launch —, antialias), which add into a tensor the host now zeroes before each pass."""
  leaves = op.fresh(op.leaves)
  out = op.forward(leaves)
  value = op.loss(out, 'weighted')
  want = op.want('weighted')
  assert float(want.heuristic.abs().max()) > 0
  for k in range(3):
    for t in leaves.values():
      t.grad = None
    op.reset(out)
    value.backward(retain_graph=True)
    check_heuristics(op, op.point_outputs(out)[1], want.heuristic, (op, f'after {k + 1} passes'))
  check_against_truth(op, leaves, op.leaves, 'weighted', (op, 'pass 3'), out=out)
