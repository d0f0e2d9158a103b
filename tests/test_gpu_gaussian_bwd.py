"""-m gpu: the fused per-gaussian backward pass (csrc/gaussian_bwd.hip) against a float64 oracle.

Part A drives the kernel ALONE through the C-ABI: ``ms_frame_project`` fills keep_n (depth, colours, camera position),
``ms_frame_backward`` with ``stage = MS_BACKWARD_GAUSSIANS`` then runs only this pass on boundary rows the test supplies.
The truth is float64 torch autograd on the CPU (tests/gaussian_bwd_oracle.py) with the same input values: axis/sigma
rows through ``oracle.projection``'s eigen chain, covariance rows through ``covariance_all``, colours through
``oracle.sh.evaluate_sh_at`` (positions and camera position detached); extras are added at the oracle's own outputs.
Every row of every output is compared (no quantiles on the covariance path, tolerance T_cov from the host build,
tests/test_hostmath.py::test_projection_backward_cov_f32_rows), outputs start as NaN with a guard row behind them,
culled rows must be exact zeros.

Scenes: ``margin = 0.6``, large splats whose projected centre is clamped, SH amplitude 2.0 (4.0 at degree 0).  On the
cases with n >= 20 000 — at least one float32 case per SH degree, and the 600 001-row case — the test asserts that a
third or more of the rows are culled (inside waves), that >= 1 % of the visible rows have a clamped centre and that
10 % .. 75 % of the visible colours are saturated, so the clamp mask matters.  The small cases (n <= 257) probe wave
and block edges; the generator sizes splats as width / sqrt(n), so few or none of their rows are culled and no share is
asserted there.

Case table (a covering selection drawn once with a seeded shuffle and kept as the literal ``CASES``; every value of
every axis occurs with every SH degree — asserted at import by ``_check_coverage``; f64 frames have no row stride /
gather; at degree -1 the pass writes no grad_feature, the pointer stays NULL):

  deg dtype f form stride gather   extras      NULL output      n
   -1   f32 4    0      0      0    depth    grad_position     64
   -1   f64 1    1      0      0      all     grad_feature    257
   -1   f32 3    1    7+f      0    depth    grad_position     63
   -1   f32 4    0     16      0     none      grad_camera      1
   -1   f32 2    0    7+f      3  colours    grad_rotation  20000
   -1   f32 2    1     16      3      all grad_alpha_logit     64
   -1   f64 3    0      0      0  colours             none    255
   -1   f32 1    1      0      0  points7 grad_log_scaling     65
    0   f32 4    1      0      0  colours      grad_camera     64
    0   f64 1    0      0      0     none grad_log_scaling     65
    0   f32 1    0    7+f      0     none    grad_rotation     63
    0   f32 2    0     16      0    depth     grad_feature      1
    0   f32 3    1    7+f      3      all    grad_rotation    257
    0   f32 4    1     16      3  points7    grad_position      1
    0   f64 3    1      0      0  points7             none    255
    0   f32 2    0      0      0      all grad_alpha_logit  20000
    1   f32 1    1      0      0     none      grad_camera     63
    1   f64 1    1      0      0  points7             none     65
    1   f32 3    0    7+f      0  points7 grad_log_scaling  20000
    1   f32 4    0     16      0  colours     grad_feature      1
    1   f32 3    1    7+f      3      all    grad_position     64
    1   f32 4    0     16      3     none grad_alpha_logit    257
    1   f64 2    0      0      0    depth      grad_camera  20000
    1   f32 2    1      0      0  colours    grad_rotation    255
    2   f32 4    1      0      0      all    grad_rotation     63
    2   f64 2    1      0      0     none    grad_rotation  20000
    2   f32 3    0    7+f      0      all grad_alpha_logit    255
    2   f32 4    1     16      0  points7             none      1
    2   f32 2    1    7+f      3     none grad_log_scaling    257
    2   f32 1    0     16      3  colours      grad_camera     65
    2   f64 1    0      0      0  colours     grad_feature    255
    2   f32 3    0      0      0    depth    grad_position     64
    2   f32 4    0      0      0  colours             none  20000
    3   f32 4    1      0      0    depth     grad_feature    255
    3   f64 4    1      0      0  points7    grad_position    257
    3   f32 1    0    7+f      0  colours grad_log_scaling      1
    3   f32 2    1     16      0      all             none  20000
    3   f32 2    0    7+f      3     none      grad_camera     65
    3   f32 3    0     16      3  points7 grad_alpha_logit     63
    3   f64 1    1      0      0    depth             none  20000
    3   f32 3    0      0      0  colours    grad_rotation     64

plus float32 RGB degree 1 and 3 at n = 20 000 with a 16-byte aligned grad_feature (128-bit stores) and the same rows
with grad_feature offset by 4 bytes (scalar stores), compared bit for bit; and one float32 case of 600 001 rows with
grad_camera, where the grid-stride loop runs twice with a ragged tail.

Part B reaches the moment-row instantiations (``MOM``, ``FIXED``) through whole frames: SH degree 0..3 x deterministic
backward off / on x point heuristics off / on, saturating features, protocol of
tests/test_gpu_configs.py::test_downscaled_config_matches_oracle_f32; and the camera-pose gradients of a frame with SH
against float64 autograd through the whole oracle pipeline."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import projection as oproj
from taichi_splatting_amd import RasterConfig, _lib
from taichi_splatting_amd.testing import random_camera
from .gaussian_bwd_oracle import (BLUR_COV, CLAMP_MARGIN, T_COV, clamp_active, clamped_centre_scene, oracle_backward,
                                  row_error, sh_features)
from .test_gpu_projection_sh import assert_f32_gradient_as_accurate_as_reference

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IMAGE_SIZE = (256, 192)
PER_ROW = ('position', 'log_scaling', 'rotation', 'alpha_logit')
WIDTH = dict(position=3, log_scaling=3, rotation=4, alpha_logit=1)

# ---- case table ------------------------------------------------------------------------------------------------------

DEGREES = (-1, 0, 1, 2, 3)
NS = (1, 63, 64, 65, 255, 257, 20000)
FS = (1, 2, 3, 4)
FORMS = (0, 1)
EXTRAS = ('none', 'points7', 'depth', 'colours', 'all')
NULLS = ('none', 'grad_position', 'grad_log_scaling', 'grad_rotation', 'grad_alpha_logit', 'grad_feature', 'grad_camera')
# (a row stride and gathered rows exist on float32 frames only, and gathered rows need a stride)
AXES = dict(dtype=('f32', 'f64'), f=FS, form=FORMS, stride=('0', '7+f', '16'), gather=(0, 3), extras=EXTRAS, null=NULLS, n=NS)


# one row per case: the table of the module docstring (``_check_coverage`` and the docstring assert keep the three in step)
CASES = [
  dict(degree=-1, dtype='f32', f=4, form=0, stride='0', gather=0, extras='depth', null='grad_position', n=64, seed=100),
  dict(degree=-1, dtype='f64', f=1, form=1, stride='0', gather=0, extras='all', null='grad_feature', n=257, seed=101),
  dict(degree=-1, dtype='f32', f=3, form=1, stride='7+f', gather=0, extras='depth', null='grad_position', n=63, seed=102),
  dict(degree=-1, dtype='f32', f=4, form=0, stride='16', gather=0, extras='none', null='grad_camera', n=1, seed=103),
  dict(degree=-1, dtype='f32', f=2, form=0, stride='7+f', gather=3, extras='colours', null='grad_rotation', n=20000, seed=104),
  dict(degree=-1, dtype='f32', f=2, form=1, stride='16', gather=3, extras='all', null='grad_alpha_logit', n=64, seed=105),
  dict(degree=-1, dtype='f64', f=3, form=0, stride='0', gather=0, extras='colours', null='none', n=255, seed=106),
  dict(degree=-1, dtype='f32', f=1, form=1, stride='0', gather=0, extras='points7', null='grad_log_scaling', n=65, seed=107),
  dict(degree=0, dtype='f32', f=4, form=1, stride='0', gather=0, extras='colours', null='grad_camera', n=64, seed=200),
  dict(degree=0, dtype='f64', f=1, form=0, stride='0', gather=0, extras='none', null='grad_log_scaling', n=65, seed=201),
  dict(degree=0, dtype='f32', f=1, form=0, stride='7+f', gather=0, extras='none', null='grad_rotation', n=63, seed=202),
  dict(degree=0, dtype='f32', f=2, form=0, stride='16', gather=0, extras='depth', null='grad_feature', n=1, seed=203),
  dict(degree=0, dtype='f32', f=3, form=1, stride='7+f', gather=3, extras='all', null='grad_rotation', n=257, seed=204),
  dict(degree=0, dtype='f32', f=4, form=1, stride='16', gather=3, extras='points7', null='grad_position', n=1, seed=205),
  dict(degree=0, dtype='f64', f=3, form=1, stride='0', gather=0, extras='points7', null='none', n=255, seed=206),
  dict(degree=0, dtype='f32', f=2, form=0, stride='0', gather=0, extras='all', null='grad_alpha_logit', n=20000, seed=207),
  dict(degree=1, dtype='f32', f=1, form=1, stride='0', gather=0, extras='none', null='grad_camera', n=63, seed=300),
  dict(degree=1, dtype='f64', f=1, form=1, stride='0', gather=0, extras='points7', null='none', n=65, seed=301),
  dict(degree=1, dtype='f32', f=3, form=0, stride='7+f', gather=0, extras='points7', null='grad_log_scaling', n=20000, seed=302),
  dict(degree=1, dtype='f32', f=4, form=0, stride='16', gather=0, extras='colours', null='grad_feature', n=1, seed=303),
  dict(degree=1, dtype='f32', f=3, form=1, stride='7+f', gather=3, extras='all', null='grad_position', n=64, seed=304),
  dict(degree=1, dtype='f32', f=4, form=0, stride='16', gather=3, extras='none', null='grad_alpha_logit', n=257, seed=305),
  dict(degree=1, dtype='f64', f=2, form=0, stride='0', gather=0, extras='depth', null='grad_camera', n=20000, seed=306),
  dict(degree=1, dtype='f32', f=2, form=1, stride='0', gather=0, extras='colours', null='grad_rotation', n=255, seed=307),
  dict(degree=2, dtype='f32', f=4, form=1, stride='0', gather=0, extras='all', null='grad_rotation', n=63, seed=400),
  dict(degree=2, dtype='f64', f=2, form=1, stride='0', gather=0, extras='none', null='grad_rotation', n=20000, seed=401),
  dict(degree=2, dtype='f32', f=3, form=0, stride='7+f', gather=0, extras='all', null='grad_alpha_logit', n=255, seed=402),
  dict(degree=2, dtype='f32', f=4, form=1, stride='16', gather=0, extras='points7', null='none', n=1, seed=403),
  dict(degree=2, dtype='f32', f=2, form=1, stride='7+f', gather=3, extras='none', null='grad_log_scaling', n=257, seed=404),
  dict(degree=2, dtype='f32', f=1, form=0, stride='16', gather=3, extras='colours', null='grad_camera', n=65, seed=405),
  dict(degree=2, dtype='f64', f=1, form=0, stride='0', gather=0, extras='colours', null='grad_feature', n=255, seed=406),
  dict(degree=2, dtype='f32', f=3, form=0, stride='0', gather=0, extras='depth', null='grad_position', n=64, seed=407),
  dict(degree=2, dtype='f32', f=4, form=0, stride='0', gather=0, extras='colours', null='none', n=20000, seed=900),
  dict(degree=3, dtype='f32', f=4, form=1, stride='0', gather=0, extras='depth', null='grad_feature', n=255, seed=500),
  dict(degree=3, dtype='f64', f=4, form=1, stride='0', gather=0, extras='points7', null='grad_position', n=257, seed=501),
  dict(degree=3, dtype='f32', f=1, form=0, stride='7+f', gather=0, extras='colours', null='grad_log_scaling', n=1, seed=502),
  dict(degree=3, dtype='f32', f=2, form=1, stride='16', gather=0, extras='all', null='none', n=20000, seed=503),
  dict(degree=3, dtype='f32', f=2, form=0, stride='7+f', gather=3, extras='none', null='grad_camera', n=65, seed=504),
  dict(degree=3, dtype='f32', f=3, form=0, stride='16', gather=3, extras='points7', null='grad_alpha_logit', n=63, seed=505),
  dict(degree=3, dtype='f64', f=1, form=1, stride='0', gather=0, extras='depth', null='none', n=20000, seed=506),
  dict(degree=3, dtype='f32', f=3, form=0, stride='0', gather=0, extras='colours', null='grad_rotation', n=64, seed=507),
]


def _case_id(c):
  return (f"deg{c['degree']}-{c['dtype']}-f{c['f']}-form{c['form']}-stride{c['stride']}-gather{c['gather']}-"
          f"extras_{c['extras']}-null_{c['null']}-n{c['n']}")


def case_table():
  head = f"  {'deg':>3} {'dtype':>5} {'f':>1} {'form':>4} {'stride':>6} {'gather':>6} {'extras':>8} {'NULL output':>16} {'n':>6}"
  lines = [head] + [f"  {c['degree']:>3} {c['dtype']:>5} {c['f']:>1} {c['form']:>4} {c['stride']:>6} {c['gather']:>6} "
                    f"{c['extras']:>8} {c['null']:>16} {c['n']:>6}" for c in CASES]
  return '\n'.join(lines)


def _check_coverage():
  for degree in DEGREES:
    mine = [c for c in CASES if c['degree'] == degree]
    for axis, values in AXES.items():
      seen = {c[axis] for c in mine}
      assert seen == set(values), (degree, axis, seen)
    # the scene conditions (culled, clamped-centre, saturated shares) are asserted at n >= 20 000: every float32
    # DEG instantiation must run under them
    assert any(c['dtype'] == 'f32' and c['n'] >= 20000 for c in mine), degree


_check_coverage()
assert case_table() in __doc__, "the case table of the module docstring is out of date:\n" + case_table()


# ---- harness: project, then the per-gaussian pass alone ----------------------------------------------------------------

class Harness:
  """One scene on the GPU: ``ms_frame_project`` into keep_n once, then any number of MS_BACKWARD_GAUSSIANS passes."""

  def __init__(self, inputs, camera, f, degree, dtype):
    self.lib = _lib.load()
    self.n, self.f, self.degree, self.dtype = inputs[0].shape[0], f, degree, dtype
    self.D = (degree + 1) ** 2 if degree >= 0 else 1
    self.dev = [t.to(dtype).contiguous().to(DEV) for t in inputs]
    w, h = camera.image_size
    cfg = RasterConfig()
    self.desc = _lib.FrameDescC(n=self.n, k_capacity=0, image_w=w, image_h=h, dtype=_lib.dtype_code(dtype), f=f,
                                sh_degree=degree, depth16=0, tile_row_begin=0, tile_row_end=(h + cfg.tile_size - 1) // cfg.tile_size,
                                projected_input=0, mapper=0, near_plane=float(camera.depth_range[0]),
                                far_plane=float(camera.depth_range[1]), blur_cov=BLUR_COV, clamp_margin=CLAMP_MARGIN,
                                raster=_lib.raster_config_c(cfg))
    self.lay = _lib.FrameLayoutC()
    _lib.check(self.lib.ms_frame_layout_query(ctypes.byref(self.desc), ctypes.byref(self.lay)), "layout")
    self.keep_n = torch.zeros((max(int(self.lay.keep_n_bytes), 1),), dtype=torch.uint8, device=DEV)
    pos, ls, rot, al, feat, T, P = self.dev
    self.inputs_c = _lib.FrameInputsC(position=pos.data_ptr(), log_scaling=ls.data_ptr(), rotation=rot.data_ptr(),
                                      alpha_logit=al.data_ptr(), feature=feat.data_ptr(), T_camera_world=T.data_ptr(),
                                      projection=P.data_ptr(), points7=None, depth=None, colours=None)
    self.stream = _lib.current_stream(torch.device(DEV))
    _lib.check(self.lib.ms_frame_project(ctypes.byref(self.desc), ctypes.byref(self.inputs_c), self.keep_n.data_ptr(),
                                         self.stream), "project")
    torch.cuda.synchronize()
    es = torch.empty((), dtype=dtype).element_size()
    view = lambda off, shape: self.keep_n[off:off + es * int(np.prod(shape))].view(dtype).view(*shape)
    self.depth = view(self.lay.depth, (self.n,)).cpu()
    self.colours = view(self.lay.colours, (self.n, f)).cpu() if degree >= 0 else None

  def backward(self, rows=None, cols=None, form=0, stride=0, gather=None, extras=None, null='none', feature_offset=False):
    """rows (n, 7) / cols (n, f): dense boundary rows (CPU tensors of the frame's dtype); stride > 0: interleaved in one
    (n, stride) array; gather = (buffer (m, stride), slots (n, world), route (n,)).  Returns the outputs on the CPU,
    guard row included: name -> (n + 1, width); camera (16,)."""
    n, f, dtype = self.n, self.f, self.dtype
    es = torch.empty((), dtype=dtype).element_size()
    g = _lib.FrameGradsC()
    g.stage = _lib.BACKWARD_GAUSSIANS
    g.boundary_form = form
    hold = []
    up = lambda t: hold.append(t.to(dtype).contiguous().to(DEV)) or hold[-1]
    if gather is not None:
      buf, slots, route = gather
      world = slots.shape[1]
      assert buf.shape[1] == stride and slots.dtype == torch.int32 and route.dtype == torch.int32
      assert int(slots.max()) < buf.shape[0] and int((route >> 16).max()) <= world     # every listed row exists
      g.gather_world, g.boundary_stride = world, stride
      g.gather_rows = up(buf).data_ptr()
      hold.append(slots.contiguous().to(DEV)); g.gather_slots = hold[-1].data_ptr()
      hold.append(route.contiguous().to(DEV)); g.gather_route = hold[-1].data_ptr()
    elif stride > 0:
      assert stride >= 7 + f
      torch.manual_seed(7)
      both = torch.randn(n, stride).to(dtype)                  # (padding columns hold noise: nobody may read them)
      both[:, :7] = rows
      both[:, 7:7 + f] = cols if cols is not None else 0
      base = up(both)
      g.boundary_stride = stride
      g.grad_points7, g.grad_colours = base.data_ptr(), base.data_ptr() + 7 * es
    else:
      g.grad_points7 = up(rows).data_ptr()
      g.grad_colours = up(cols).data_ptr() if cols is not None else None
    extras = extras or {}
    for name in ('extra_points7', 'extra_depth', 'extra_colours'):
      if extras.get(name) is not None:
        setattr(g, name, up(extras[name]).data_ptr())
    nan = lambda *shape: torch.full(shape, float('nan'), dtype=dtype, device=DEV)
    out = {name: nan(n + 1, WIDTH[name]) for name in PER_ROW}
    if self.degree >= 0:
      flat = nan((n + 1) * f * self.D + 4)
      out['feature'] = flat[1:1 + (n + 1) * f * self.D] if feature_offset else flat[:(n + 1) * f * self.D]
      assert (out['feature'].data_ptr() % 16 == 4) == bool(feature_offset)
    out['camera'] = torch.zeros(16, dtype=dtype, device=DEV)      # the 16 camera sums are accumulated into
    for name, t in out.items():
      if null != 'grad_' + name:
        setattr(g, 'grad_' + name, t.data_ptr())
    _lib.check(self.lib.ms_frame_backward(ctypes.byref(self.desc), ctypes.byref(self.inputs_c), self.keep_n.data_ptr(), None,
                                          ctypes.byref(g), self.stream), "per-gaussian backward")
    torch.cuda.synchronize()
    res = {name: t.cpu() for name, t in out.items() if null != 'grad_' + name}
    if 'feature' in res:
      res['feature'] = res['feature'].reshape(n + 1, f * self.D)
    return res


def make_scene(n, f, degree, dtype, seed):
  torch.manual_seed(seed)
  camera = random_camera(image_size=IMAGE_SIZE)
  g = clamped_centre_scene(n, camera, scale_factor=1.0, margin=0.6)
  feature = sh_features(n, f, degree)
  inputs = [t.to(dtype) for t in (*g.shape_tensors(), feature, camera.T_camera_world, camera.projection)]
  return camera, inputs


def make_gather(n, f, stride, common, dtype, seed, world=3):
  """Receive buffer of a rank step's reverse exchange: 0..3 copies per gaussian in ``route >> 16`` (noise in the low
  half), their rows a random permutation of the buffer, some slots -1 (dropped copies), spare rows nobody lists."""
  gen = torch.Generator().manual_seed(seed)
  copies = torch.randint(0, world + 1, (n,), generator=gen) * common.long()
  total = int(copies.sum())
  m = total + 7
  buf = torch.randn(m, stride, generator=gen).to(dtype)
  perm = torch.randperm(m, generator=gen)[:total]
  slots = torch.full((n, world), -1, dtype=torch.int64)
  listed = torch.arange(world).unsqueeze(0) < copies.unsqueeze(1)
  slots[listed] = perm
  dropped = listed & (torch.rand(n, world, generator=gen) < 0.1)
  slots[dropped] = -1
  route = ((copies << 16) | torch.randint(0, 1 << 15, (n,), generator=gen)).to(torch.int32)
  # what the pass must see: the listed rows summed — in float64 for the oracle, in the frame's dtype and in copy order
  # for the dense-array twin
  exact = torch.zeros(n, 7 + f, dtype=torch.float64)
  ordered = torch.zeros(n, 7 + f, dtype=dtype)
  for c in range(world):
    use = (slots[:, c] >= 0) & (c < copies)
    picked = buf[slots[:, c].clamp(min=0)][:, :7 + f] * use.unsqueeze(1)
    exact += picked.double()
    ordered = ordered + picked
  return (buf, slots.to(torch.int32), route), exact, ordered


def check_pass(h, out, vis, null, label):
  """NaN-filled outputs: rows 0..n-1 all written, culled rows exact zeros, the guard row untouched"""
  n = h.n
  for name, t in out.items():
    if name == 'camera':
      assert torch.isfinite(t).all(), (label, name)
      continue
    assert not torch.isnan(t[:n]).any(), (label, name, 'unwritten rows', int(torch.isnan(t[:n]).any(dim=1).sum()))
    assert torch.isnan(t[n]).all(), (label, name, 'wrote beyond row n - 1')
    assert (t[:n][~vis] == 0).all(), (label, name, 'culled rows must be zero')


def compare_with_oracle(h, out, want, ref32, cov_path, vis, g_col_scale, label, sample=None):
  f32 = h.dtype == torch.float32
  n = h.n
  pick = (lambda t: t[:n]) if sample is None else (lambda t: t[:n][sample])
  for name in PER_ROW:
    if name not in out:
      continue
    got, w64 = pick(out[name]).reshape(-1, WIDTH[name]), pick(want[name]).reshape(-1, WIDTH[name])
    if not f32:
      assert torch.allclose(got, w64, rtol=1e-5, atol=1e-9), (label, name, float((got - w64).abs().max()))
    elif float(want[name].abs().max()) == 0.0:
      assert (got == 0).all(), (label, name)
    elif cov_path:
      err = row_error(got, w64) * float(w64.abs().max()) / float(want[name].abs().max())
      print(f"{label}: {name} worst row {float(err.max()):.2e} (T_cov {T_COV:.1e})")
      assert float(err.max()) <= T_COV, (label, name, float(err.max()), int(err.argmax()))
    else:
      assert_f32_gradient_as_accurate_as_reference(got, w64, pick(ref32[name]).reshape(-1, WIDTH[name]), (label, name))
  if 'camera' in out:
    got, w64 = out['camera'].double(), want['camera']
    if not f32:
      assert torch.allclose(got, w64, rtol=1e-5, atol=1e-9 * max(1.0, float(w64.abs().max()))), (label, 'camera', got, w64)
    elif float(w64.abs().max()) > 0:
      # the existing rule for sums over all gaussians: error <= 5 x the float32 oracle's + 1e-5 of the largest entry
      assert_f32_gradient_as_accurate_as_reference(out['camera'], w64, ref32['camera'], (label, 'camera'))
  if 'feature' in out and h.degree >= 0:
    D = h.D
    got = pick(out['feature']).reshape(-1, h.f, D).double()
    w64 = pick(want['feature']).reshape(-1, h.f, D)
    pre = want['pre_clamp']
    near = ((pre.abs() < 1e-6) | ((pre - 1).abs() < 1e-6)) & vis.unsqueeze(1)
    share = float(near.sum()) / max(1, int(vis.sum()) * h.f)
    # entries whose float64 colour lies within 1e-6 of 0 or 1 may disagree on the clamp mask: at most 0.1 % of them
    assert share <= 1e-3, (label, 'colours within 1e-6 of the clamp', int(near.sum()))
    keep = ~pick(near)
    if f32:
      bad = ((got - w64).abs() > 1e-5 * max(g_col_scale, 1e-30)) & keep.unsqueeze(2)
    else:
      bad = ~torch.isclose(got, w64, rtol=1e-5, atol=1e-10) & keep.unsqueeze(2)
    assert not bad.any(), (label, 'feature', int(bad.sum()), 'entries off; largest', float(((got - w64).abs() * keep.unsqueeze(2)).max()),
                           'near-clamp entries excluded:', int(near.sum()))


def run_case(c, feature_offset_twin=False):
  dtype = torch.float32 if c['dtype'] == 'f32' else torch.float64
  n, f, degree, form = c['n'], c['f'], c['degree'], c['form']
  label = _case_id(c)
  camera, inputs = make_scene(n, f, degree, dtype, c['seed'])
  h = Harness(inputs, camera, f, degree, dtype)
  in64 = [t.double() for t in inputs]

  # the visible set: the kernel's (depth > 0) against the float64 oracle's; a float32 culling flip on the frustum edge
  # is allowed max(1, n // 2000) times, and the upstream rows outside the common set are zeroed
  vis = h.depth > 0
  with torch.no_grad():
    _, _, in_view = oproj.project_all(*in64[:4], in64[5], in64[6], camera.image_size, camera.depth_range,
                                      blur_cov=BLUR_COV, clamp_margin=CLAMP_MARGIN)
  flips = int((vis ^ in_view).sum())
  assert flips <= max(1, n // 2000), (label, 'culling flips', flips)
  common = vis & in_view
  idx = common.nonzero(as_tuple=True)[0]
  if n >= 20000:
    assert float((~vis).double().mean()) >= 1 / 3, (label, 'culled share', float((~vis).double().mean()))
    clamped = clamp_active(in64[0], in64[5], in64[6], camera.image_size)[idx]
    assert float(clamped.double().mean()) >= 0.01, (label, 'clamped-centre share', float(clamped.double().mean()))

  torch.manual_seed(c['seed'] + 50000)
  mask = common.unsqueeze(1)
  rows = (torch.randn(n, 7) * mask).to(dtype)
  if form == 1:
    rows[:, 5] = 0
  cols = (torch.randn(n, f) * mask).to(dtype)
  kinds = {'none': (), 'points7': ('extra_points7',), 'depth': ('extra_depth',), 'colours': ('extra_colours',),
           'all': ('extra_points7', 'extra_depth', 'extra_colours')}[c['extras']]
  extras = {}
  if 'extra_points7' in kinds:
    extras['extra_points7'] = (torch.randn(n, 7) * mask).to(dtype)
  if 'extra_depth' in kinds:
    extras['extra_depth'] = (torch.randn(n) * common).to(dtype)
  if 'extra_colours' in kinds:
    extras['extra_colours'] = (torch.randn(n, f) * mask).to(dtype)

  stride = {'0': 0, '7+f': 7 + f, '16': 16}[c['stride']]
  gather = None
  rows64, cols64 = rows.double(), cols.double()
  if c['gather']:
    gather, exact, ordered = make_gather(n, f, stride, common, dtype, c['seed'] + 9, world=c['gather'])
    rows64, cols64 = exact[:, :7].clone(), exact[:, 7:].clone()
    rows, cols = ordered[:, :7].contiguous(), ordered[:, 7:].contiguous()          # the dense twin's inputs
    if form == 1:
      gather[0][:, 5] = 0; rows64[:, 5] = 0; rows[:, 5] = 0

  # ---- oracle (float64 truth; float32 = the reference's own arithmetic as yardstick) ----------------------------------
  ep7 = extras.get('extra_points7')
  g_points7 = (rows64 + (ep7.double() if ep7 is not None else 0)) if form == 0 else (ep7.double() if ep7 is not None else None)
  g_cov_rows = rows64 if form == 1 else None
  g_depth = extras['extra_depth'].double() if 'extra_depth' in extras else None
  g_col = None
  if degree >= 0:
    g_col = cols64 + (extras['extra_colours'].double() if 'extra_colours' in extras else 0)
  kw = dict(g_points7=g_points7, g_cov_rows=g_cov_rows, g_depth=g_depth, g_colours=g_col, sh_degree=degree)
  want = oracle_backward(in64, camera.image_size, idx, **kw)
  ref32 = oracle_backward(inputs, camera.image_size, idx, dtype=torch.float32, **kw) if dtype == torch.float32 else None
  if degree >= 0 and n >= 20000:
    pre = want['pre_clamp'][idx]
    saturated = float(((pre <= 0) | (pre >= 1)).double().mean())
    assert 0.10 <= saturated <= 0.75, (label, 'saturated colours', saturated)

  # ---- the kernel ------------------------------------------------------------------------------------------------------
  null = c['null'] if not (degree < 0 and c['null'] == 'grad_feature') else 'none'
  out = h.backward(rows, cols, form=form, stride=stride, gather=gather, extras=extras, null=null)
  check_pass(h, out, vis, null, label)
  cov_path = form == 1 and ep7 is None
  sample = c.get('sample')
  compare_with_oracle(h, out, want, ref32, cov_path, vis, float(g_col.abs().max()) if g_col is not None else 0.0, label, sample)

  # a row stride / gathered rows must give what the dense arrays of the same rows give, bit for bit (gathered copies
  # are summed in the frame's dtype in copy order: the twin's rows are that sum)
  if stride > 0 or gather is not None:
    twin = h.backward(rows, cols, form=form, stride=0, gather=None, extras=extras, null=null)
    for name in out:
      if name != 'camera':        # (float atomics: the 16 sums arrive in another order)
        assert torch.equal(out[name][:n], twin[name][:n]), (label, name, 'differs from the dense-array result')
  if feature_offset_twin:
    twin = h.backward(rows, cols, form=form, stride=stride, gather=gather, extras=extras, null=null, feature_offset=True)
    check_pass(h, twin, vis, null, label + ' (grad_feature + 4 bytes)')
    assert torch.equal(out['feature'][:n], twin['feature'][:n]), (label, '128-bit store path differs from the scalar stores')
    assert (out['feature'][:n] != 0).any()


@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_gaussian_bwd_given_rows_vs_oracle(case):
  run_case(case)


@pytest.mark.parametrize('degree', [1, 3])
@pytest.mark.parametrize('form', [0, 1])
def test_gaussian_bwd_rgb_vector_store_path(degree, form):
  """float32 RGB, degree 1 / 3 (D = 4 / 16): the wave's SH rows leave as 128-bit stores when grad_feature is 16-byte
  aligned.  Against the oracle, and bit for bit against the scalar stores (grad_feature offset by 4 bytes)."""
  run_case(dict(degree=degree, dtype='f32', f=3, form=form, stride='0', gather=0, extras='colours', null='none',
                n=20000, seed=7000 + degree + 10 * form), feature_offset_twin=True)
  run_case(dict(degree=degree, dtype='f32', f=3, form=form, stride='7+f', gather=3, extras='none', null='grad_camera',
                n=257, seed=7100 + degree + 10 * form), feature_offset_twin=True)


def test_gaussian_bwd_grid_stride_loop_runs_twice():
  """grad_camera caps the grid at 2048 blocks of 256 gaussians: at n = 600 001 the grid-stride loop runs a second time
  with a ragged tail (rows 524 288 .. 600 000).  Per-row leaves on a seeded sample of 50 000 rows plus the first and
  last 512; NaN / zero / guard checks and the camera sums in full."""
  n = 600_001
  gen = torch.Generator().manual_seed(3)
  sample = torch.cat([torch.arange(512), torch.randperm(n, generator=gen)[:50_000], torch.arange(n - 512, n)]).unique()
  assert int((sample >= 2048 * 256).sum()) > 1000
  run_case(dict(degree=1, dtype='f32', f=3, form=1, stride='0', gather=0, extras='depth', null='none', n=n, seed=8000,
                sample=sample))


# ---- Part B: the moment-row instantiations (MOM, FIXED) behind the raster backward of a whole frame -------------------

FRAME_N, FRAME_SIZE, FRAME_TILE = 5_860, (128, 128), 16        # config E at 1/32 scale ('E/32' of test_gpu_configs.py)


def _frame_scene(degree):
  from .test_gpu_configs import gate_stable, scene
  cfg = RasterConfig(tile_size=FRAME_TILE, pixel_stride=(2, 2))
  g, cam = scene(FRAME_N, FRAME_SIZE, seed=1, sh_degree=degree)
  torch.manual_seed(40 + degree)
  g = g.replace(feature=sh_features(FRAME_N, 3, degree))         # saturating amplitude: the clamp mask is live
  return gate_stable(g, cam, cfg), cam


_stale_moments = set()


def _frame_backward(g, cam, cfg, G, camera_grads=False):
  """One frame on the GPU with loss sum(image * G); returns the leaves, the camera, and the oracle rasterizer's float64
  2D-boundary gradients on the kernels' own splats (protocol of test_downscaled_config_matches_oracle_f32)."""
  from dataclasses import replace
  from oracle import mapper as omap, raster as orast
  from taichi_splatting_amd import render_gaussians
  from taichi_splatting_amd import frame
  frame.release_caches()          # no moments accumulator of an earlier test may stand in for this frame's
  _stale_moments.clear()
  _stale_moments.update(frame._moments)          # (only accumulators pinned by a captured graph survive the release)
  gd = g.to(DEV).requires_grad_(True)
  cam_d = cam.to(device=DEV)
  if camera_grads:
    cam_d = replace(cam_d, T_camera_world=cam_d.T_camera_world.clone().requires_grad_(True),
                    projection=cam_d.projection.clone().requires_grad_(True))
  r = render_gaussians(gd, cam_d, cfg, use_sh=True)
  r.points.gaussians2d.retain_grad()
  r.points.features.retain_grad()
  (r.image * G.to(DEV).float()).sum().backward()
  torch.cuda.synchronize()
  size = cam.image_size
  p_h, f_h = r.points.gaussians2d.detach().cpu().double(), r.points.features.detach().cpu().double()
  ndc = oproj.ndc_depth(r.points.depths.detach().cpu().double(), *cam.depth_range)
  o2p_h, ranges_h = omap.map_to_tiles(p_h.numpy().astype(np.float32), ndc.numpy().astype(np.float32), size, cfg.tile_size,
                                      cfg.alpha_threshold)[:2]
  o2p_h, ranges_h = torch.from_numpy(o2p_h), torch.from_numpy(ranges_h)
  assert float(orast.gate_margin(p_h, ranges_h, o2p_h, size, cfg).min()) > 1e-4        # gate-stable on the kernels' inputs
  img_h, _, _ = orast.forward(p_h, f_h, ranges_h, o2p_h, size, cfg)
  gp_h, gf_h, _ = orast.backward(p_h, f_h, ranges_h, o2p_h, img_h, G, size, cfg)
  gp_k, gf_k = r.points.gaussians2d.grad.cpu().double(), r.points.features.grad.cpu().double()
  # the raster backward's share first (1e-4 of the largest 2D gradient, every row): a failure further down then
  # belongs to the per-gaussian pass
  assert float((r.image.detach().cpu().double() - img_h).abs().max()) < 1e-4
  for k, got, w in (('gaussians2d', gp_k, gp_h), ('features', gf_k, gf_h)):
    assert float((got - w).abs().max()) < 1e-4 * float(w.abs().max()), (k, float((got - w).abs().max()), float(w.abs().max()))
  saturated = float(((f_h <= 0) | (f_h >= 1)).double().mean())
  assert 0.10 <= saturated <= 0.75, ('saturated colours', saturated)
  return gd, cam_d, r.points.idx.cpu(), p_h, (gp_h, gf_h), (gp_k, gf_k)


def _assert_moments_buffer_clean(n, deterministic):
  """include/mi355_splat.h: the moment rows are "zero again on return" — the next frame accumulates into them"""
  from taichi_splatting_amd import frame
  device = torch.device(DEV)
  key = (device.index, int(torch.cuda.current_stream(device).cuda_stream), int(n), bool(deterministic))
  assert key in frame._moments and key not in _stale_moments, "the frame did not take the moments path"
  buf = frame._moments_buffer(device, n, deterministic)
  assert buf.dtype == (torch.int64 if deterministic else torch.float32)
  assert int(buf.view(torch.int32).ne(0).sum()) == 0, "moment rows are not all-zero bytes after the backward"


@pytest.mark.parametrize('heuristic', [False, True])
@pytest.mark.parametrize('deterministic', [False, True])
@pytest.mark.parametrize('degree', [0, 1, 2, 3])
def test_moment_rows_frame_matches_oracle(degree, deterministic, heuristic, monkeypatch):
  """gaussian_bwd_kernel<float, DEG, MOM, FIXED> for every SH degree, float and fixed-point moment rows, with and
  without the heuristics columns.  Truth: the float64 oracle rasterizer's gradient on the kernels' own splats pushed
  through the float64 chain as a covariance gradient; criterion: assert_f32_gradient_as_accurate_as_reference for the
  five leaves — the deterministic mode on its own, not relative to the plain run."""
  from taichi_splatting_amd.rasterizer import function as raster_function
  from .test_gpu_configs import LEAVES, oracle_leaf_grads, oracle_leaf_grads_from_covariance
  monkeypatch.setattr(raster_function, 'DETERMINISTIC_BACKWARD', deterministic)
  cfg = RasterConfig(tile_size=FRAME_TILE, pixel_stride=(2, 2), compute_point_heuristic=heuristic)
  g, cam = _frame_scene(degree)
  torch.manual_seed(2)
  G = torch.rand(FRAME_SIZE[1], FRAME_SIZE[0], 3, dtype=torch.float64) + 0.5
  gd, _, idx, p_h, (gp_h, gf_h), (gp_k, gf_k) = _frame_backward(g, cam, cfg, G)
  _assert_moments_buffer_clean(g.position.shape[0], deterministic)
  idx64, ref64 = oracle_leaf_grads_from_covariance(g, cam, cfg, p_h, gp_h, gf_h)
  idx32, ref32 = oracle_leaf_grads(g, cam, cfg, gp_k, gf_k, torch.float32)
  assert torch.equal(idx64, idx) and torch.equal(idx32, idx)
  for k, w64, w32 in zip(LEAVES, ref64, ref32):
    assert_f32_gradient_as_accurate_as_reference(getattr(gd, k).grad.cpu(), w64, w32, (degree, deterministic, heuristic, k))


@pytest.mark.parametrize('deterministic', [False, True])
@pytest.mark.parametrize('degree', [1, 3])
def test_frame_camera_pose_gradients_with_sh_match_oracle(degree, deterministic, monkeypatch):
  """T_camera_world and projection require grad, SH on: the colours depend on the camera position =
  inverse(T_camera_world)[:3, 3], NOT detached (the ``sh_camera`` branch of frame.py).  Truth: float64 autograd through
  the oracle's projection + SH chain with the camera as a leaf; rule for sums over all gaussians: error <= 5 x the
  float32 oracle's + 1e-5 of the largest entry."""
  from dataclasses import replace
  from taichi_splatting_amd.rasterizer import function as raster_function
  from .test_gpu_configs import oracle_leaf_grads, oracle_leaf_grads_from_covariance
  monkeypatch.setattr(raster_function, 'DETERMINISTIC_BACKWARD', deterministic)
  cfg = RasterConfig(tile_size=FRAME_TILE, pixel_stride=(2, 2))
  g, cam = _frame_scene(degree)
  torch.manual_seed(3)
  G = torch.rand(FRAME_SIZE[1], FRAME_SIZE[0], 3, dtype=torch.float64) + 0.5
  gd, cam_d, idx, p_h, (gp_h, gf_h), (gp_k, gf_k) = _frame_backward(g, cam, cfg, G, camera_grads=True)
  _assert_moments_buffer_clean(g.position.shape[0], deterministic)
  leaf = lambda dtype: replace(cam, T_camera_world=cam.T_camera_world.to(dtype).clone().requires_grad_(True),
                               projection=cam.projection.to(dtype).clone().requires_grad_(True))
  cam64, cam32 = leaf(torch.float64), leaf(torch.float32)
  oracle_leaf_grads_from_covariance(g, cam64, cfg, p_h, gp_h, gf_h)
  oracle_leaf_grads(g, cam32, cfg, gp_k, gf_k, torch.float32)
  for name in ('T_camera_world', 'projection'):
    got, w64, w32 = getattr(cam_d, name).grad.cpu(), getattr(cam64, name).grad, getattr(cam32, name).grad
    assert w64 is not None and float(w64.abs().max()) > 0
    assert_f32_gradient_as_accurate_as_reference(got.reshape(-1), w64.reshape(-1), w32.reshape(-1), (degree, deterministic, name))
