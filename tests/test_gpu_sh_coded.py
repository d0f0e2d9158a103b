"""``evaluate_sh_coded`` / ``render_compressed`` (csrc/sh_coded.hip) against the float64 oracle of tests/sh_coded_oracle.py.

Bounds.  Colours: atol 1e-5, the project's float32 SH tolerance (tests/test_gpu_projection_sh.py).  ``g_dc``: rtol 1e-6
wherever the clamp masks agree (one float32 product of g and the rounded Y_0: 1.2e-7 relative).  ``g_codebook``:
``|got - want| <= 2e-6 S_c[j] + 1e-6 |want|`` with ``S_c[j]`` the sum of |g_c| over the members of code j: the sum of
the products is exact in float64, the only float32 error is the basis.  The float32 basis against the float64 one on the
CPU, over the directions of the cases below (``sh_coded_oracle.basis_error``): at most 4.6e-7 absolute (degree 3,
N = 257; 1.9e-7 at degree 2, 7.6e-8 at degree 1; a second CPU gave 3.2e-7, 1.6e-7 and 6.7e-8: torch's vector paths
differ), inside the 6.9e-7 measured over 6 M directions at three scales that the 2e-6 is three times of.
``test_basis_error_of_the_test_directions`` recomputes it on every run and holds it to half the 2e-6.
"""
import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from taichi_splatting_amd import (CompressedScene, RasterConfig, _lib, compress_scene, evaluate_sh_at, evaluate_sh_coded,
                                  make_coded_sh_plan, render_compressed, render_gaussians, save_ply)
from taichi_splatting_amd.testing import random_3d_gaussians, random_camera

from tests import sh_coded_oracle as oracle

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ROOT = Path(__file__).resolve().parent.parent
C = _lib.SH_CODED_CHUNK
SIZES = [(1, 1), (257, 7), (3000, 300)]
BASIS_BOUND = 1e-6        # half of the 2e-6 the codebook gradient is allowed per unit of |g| (measured: 4.6e-7 at most)

_cases = {}


def case(n, k, degree, index=None, seed=None):
  """the CPU inputs, their float64 reference (computed once, never modified) and the inputs on the GPU"""
  key = (n, k, degree, seed)
  if key not in _cases:
    cpu = oracle.random_case(n, k, degree, seed=1000 * degree + n if seed is None else seed, index=index)
    want = oracle.reference(cpu['dc'], cpu['index'], cpu['codebook'], cpu['positions'], cpu['cam'], cpu['g_out'])
    _cases[key] = (cpu, want)
  cpu, want = _cases[key]
  gpu = {name: (t.to(DEV) if isinstance(t, torch.Tensor) else t) for name, t in cpu.items()}
  return cpu, want, gpu


def run(gpu, plan=None, g_out=None):
  """forward + backward: (out, g_dc, g_codebook)"""
  dc, codebook = gpu['dc'].clone().requires_grad_(True), gpu['codebook'].clone().requires_grad_(True)
  out = evaluate_sh_coded(dc, gpu['index'], codebook, gpu['positions'], gpu['cam'], plan=plan)
  out.backward(gpu['g_out'] if g_out is None else g_out)
  return out.detach(), dc.grad, codebook.grad


def check_gradients(out, g_dc, g_codebook, want, index):
  """the bounds of the module docstring; ``out`` is the float32 colour whose clamp mask the kernels applied"""
  out, g_dc, g_codebook = out.double().cpu(), g_dc.double().cpu(), g_codebook.double().cpu()
  got_mask, want_mask = (out > 0) & (out < 1), (want['pre'] > 0) & (want['pre'] < 1)
  differ = got_mask != want_mask
  edge = torch.minimum(want['pre'].abs(), (want['pre'] - 1).abs())
  print(f"clamp masks differ in {int(differ.sum())} of {differ.numel()} pairs; closest |pre| or |pre - 1|: {float(edge.min()):.3e}")
  assert bool((edge[differ] < 1e-5).all()) and int(differ.sum()) <= 1e-3 * differ.numel()
  same = ~differ
  err_dc = (g_dc - want['g_dc']).abs()
  print(f"g_dc: max relative error {float((err_dc[same] / want['g_dc'].abs().clamp_min(1e-300)[same]).max()):.3e}")
  assert bool((err_dc[same] <= 1e-6 * want['g_dc'].abs()[same]).all())
  # a (code, channel) sum is held to its bound unless one of its members sits on the other side of the clamp
  index = index.cpu().long()
  k = g_codebook.shape[0]
  agrees = torch.zeros((k, 3), dtype=torch.float64).index_add_(0, index, differ.double()) == 0
  bound = 2e-6 * want['s'].unsqueeze(2) + 1e-6 * want['g_codebook'].abs()
  err = (g_codebook - want['g_codebook']).abs()
  print(f"g_codebook: max error / bound {float((err / bound.clamp_min(1e-300))[agrees].max()):.3e} over "
        f"{int(agrees.sum())} of {agrees.numel()} (code, channel) sums")
  assert bool((err <= bound)[agrees].all())
  assert bool((g_codebook[torch.bincount(index, minlength=k) == 0] == 0).all())


@pytest.mark.parametrize('degree', [1, 2, 3])
def test_basis_error_of_the_test_directions(degree):
  for n, k in SIZES:
    cpu, _, _ = case(n, k, degree)
    err = oracle.basis_error(cpu['positions'], cpu['cam'], degree)
    print(f"degree {degree}, N = {n}: float32 basis within {err:.3e} of float64")
    assert err <= BASIS_BOUND


@pytest.mark.parametrize('n,k', SIZES)
@pytest.mark.parametrize('degree', [1, 2, 3])
def test_forward_and_backward_against_the_oracle(degree, n, k):
  cpu, want, gpu = case(n, k, degree)
  if n >= 257:
    assert bool((want['out'] == 0).any()) and bool((want['out'] == 1).any()) and bool(((want['out'] > 0) & (want['out'] < 1)).any())
    clamped = float(((want['out'] == 0) | (want['out'] == 1)).double().mean())
    assert 0.2 < clamped < 0.6, clamped
  # the chosen seeds keep every colour 1e-4 away from the clamp's corners: the float32 mask is the float64 one
  assert float(torch.minimum(want['pre'].abs(), (want['pre'] - 1).abs()).min()) > 1e-4
  out, g_dc, g_codebook = run(gpu)
  assert out.shape == (n, 3) and out.dtype == torch.float32 and g_dc.shape == (n, 3) and g_codebook.shape == gpu['codebook'].shape
  err = float((out.double().cpu() - want['out']).abs().max())
  print(f"colours: max error {err:.3e}")
  assert err <= 1e-5
  decoded = CompressedScene(position=gpu['positions'], log_scaling=torch.zeros((n, 3), device=DEV),
                            rotation=torch.zeros((n, 4), device=DEV), alpha_logit=torch.zeros((n, 1), device=DEV),
                            dc=gpu['dc'], sh_codebook=gpu['codebook'], sh_index=gpu['index'], sh_degree=degree).decode()
  through_decode = evaluate_sh_at(decoded.feature, gpu['positions'], torch.arange(n, device=DEV), gpu['cam'])
  assert float((out - through_decode).abs().max()) <= 1e-5
  check_gradients(out, g_dc, g_codebook, want, gpu['index'])


def chunk_edge_index():
  """codes with 0, 1, C - 1, C, C + 1 and 3 C + 5 members, interleaved in storage order"""
  members = [0, 1, C - 1, C, C + 1, 3 * C + 5]
  index = torch.cat([torch.full((m,), j, dtype=torch.int32) for j, m in enumerate(members)])
  return index[torch.randperm(index.shape[0], generator=torch.Generator().manual_seed(5))].contiguous(), len(members)


def sparse_index():
  """K = 65 536 with N = 70 000: most codes are empty, a few hold many"""
  gen = torch.Generator().manual_seed(6)
  some = torch.randint(0, 65536, (30000,), generator=gen, dtype=torch.int32)
  few = torch.randint(0, 40, (40000,), generator=gen, dtype=torch.int32) * 1601 + 7
  index = torch.cat([some, few])
  index[0], index[1] = 0, 65535
  return index[torch.randperm(70000, generator=gen)].contiguous(), 65536


@pytest.mark.parametrize('name', ['edges', 'one_code', 'sparse'])
def test_chunk_edges(name):
  """degree 3; the operator's gradient through autograd, and the bare C call into a NaN-filled g_codebook: every row is
  written, the rows of empty codes as exact zeros"""
  if name == 'edges':
    index, k = chunk_edge_index()
  elif name == 'one_code':
    index, k = torch.zeros((2 * C + 3,), dtype=torch.int32), 1
  else:
    index, k = sparse_index()
  n = index.shape[0]
  cpu, want, gpu = case(n, k, 3, index=index, seed={'edges': 11, 'one_code': 12, 'sparse': 13}[name])
  plan = make_coded_sh_plan(gpu['index'], k)
  counts = torch.bincount(index.long(), minlength=k)
  assert plan.num_chunks == int(((counts + C - 1) // C).sum())
  out, g_dc, g_codebook = run(gpu, plan=plan)
  assert float((out.double().cpu() - want['out']).abs().max()) <= 1e-5
  check_gradients(out, g_dc, g_codebook, want, gpu['index'])

  from taichi_splatting_amd import spherical_harmonics as shm
  import ctypes
  filled = torch.full((k, 3, 15), float('nan'), device=DEV)
  nbytes = ctypes.c_size_t(0)
  _lib.check(shm._coded_bwd(plan, 3, None, None, None, None, None, None, None, nbytes), "query")
  tmp = torch.empty((max(nbytes.value, 1),), dtype=torch.uint8, device=DEV)
  nbytes = ctypes.c_size_t(tmp.numel())
  _lib.check(shm._coded_bwd(plan, 3, gpu['positions'], gpu['cam'], out, gpu['g_out'], None, filled, tmp, nbytes), "bare backward")
  torch.cuda.synchronize()
  assert bool(torch.isfinite(filled).all()) and torch.equal(filled, g_codebook)
  assert bool((filled[(counts == 0).to(DEV)] == 0).all())


def test_empty_scene_and_out_of_range_index_stay_in_bounds():
  """n == 0 launches nothing and gives a zero codebook gradient; an index past K is clamped by the kernel (the Python
  layer refuses it when it builds the plan)"""
  _, _, gpu = case(257, 7, 3)
  empty = {name: (t[:0] if isinstance(t, torch.Tensor) and name not in ('codebook', 'cam') else t) for name, t in gpu.items()}
  out, g_dc, g_codebook = run(empty)
  assert out.shape == (0, 3) and g_dc.shape == (0, 3) and bool((g_codebook == 0).all())
  with pytest.raises(ValueError, match="0..6"):
    evaluate_sh_coded(gpu['dc'], gpu['index'] + 1, gpu['codebook'], gpu['positions'], gpu['cam'])
  clamped = torch.empty((257, 3), device=DEV)
  bad = (gpu['index'] + 1).contiguous()
  _lib.check(_lib.load().ms_sh_coded_fwd(gpu['dc'].data_ptr(), bad.data_ptr(), gpu['codebook'].data_ptr(), gpu['positions'].data_ptr(),
                                         gpu['cam'].data_ptr(), 257, 7, 3, clamped.data_ptr(), _lib.current_stream(DEV)), "fwd")
  want = evaluate_sh_coded(gpu['dc'], bad.clamp(max=6), gpu['codebook'], gpu['positions'], gpu['cam'])
  assert torch.equal(clamped, want)


def test_backward_is_reproducible_and_captures_into_a_graph():
  _, _, gpu = case(3000, 300, 3)
  plan = make_coded_sh_plan(gpu['index'], 300)              # before capture: the plan reads the chunk count on the host
  first, second = run(gpu, plan=plan), run(gpu, plan=plan)
  for a, b in zip(first, second):
    assert torch.equal(a, b)

  dc, codebook = gpu['dc'].clone().requires_grad_(True), gpu['codebook'].clone().requires_grad_(True)
  stream = torch.cuda.Stream()
  stream.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(stream):                           # warm-up on the side stream, as torch asks before a capture
    evaluate_sh_coded(dc, gpu['index'], codebook, gpu['positions'], gpu['cam'], plan=plan).backward(gpu['g_out'])
  torch.cuda.current_stream().wait_stream(stream)
  dc.grad = codebook.grad = None
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out = evaluate_sh_coded(dc, gpu['index'], codebook, gpu['positions'], gpu['cam'], plan=plan)
    out.backward(gpu['g_out'])
  for _ in range(2):
    dc.grad.fill_(float('nan'))
    codebook.grad.fill_(float('nan'))
    out.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip((out, dc.grad, codebook.grad), first):
      assert torch.equal(got, want)


def test_no_decoded_tensor_is_allocated():
  n, k = 200_000, 256
  gen = torch.Generator(device=DEV).manual_seed(3)
  dc = (torch.randn((n, 3), device=DEV, generator=gen) * 0.5).requires_grad_(True)
  codebook = (torch.randn((k, 3, 15), device=DEV, generator=gen) * 0.5).requires_grad_(True)
  index = torch.randint(0, k, (n,), device=DEV, generator=gen, dtype=torch.int32)
  positions, cam = torch.randn((n, 3), device=DEV, generator=gen), torch.tensor([0.0, 0.0, -6.0], device=DEV)
  g_out = torch.randn((n, 3), device=DEV, generator=gen)
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats(DEV)
  before = torch.cuda.memory_allocated(DEV)
  out = evaluate_sh_coded(dc, index, codebook, positions, cam)          # the plan is built here too
  out.backward(g_out)
  torch.cuda.synchronize()
  rise = torch.cuda.max_memory_allocated(DEV) - before
  print(f"peak rise {rise} bytes = {rise / n:.1f} per gaussian; the decoded feature alone is {n * 48 * 4}")
  assert rise < n * 48 * 4
  assert dc.grad.shape == (n, 3) and codebook.grad.shape == (k, 3, 15)


def renderer_scene():
  torch.manual_seed(21)
  cam = random_camera(image_size=(160, 96))
  g = random_3d_gaussians(2000, cam, scale_factor=1.0, alpha_range=(0.1, 0.9))
  g = g.replace(feature=(torch.rand(2000, 3, 16) - 0.5) * 1.5).to(DEV)
  return compress_scene(g, sh_codes=32, iterations=5, seed=1), cam.to(device=DEV)


def test_through_the_renderer():
  scene, cam = renderer_scene()
  config = RasterConfig()
  with torch.no_grad():
    image = render_compressed(scene, cam, config).image
    decoded = render_gaussians(scene.decode(), cam, config, use_sh=True).image
  assert image.shape == (96, 160, 3)
  err = float((image - decoded).abs().max())
  print(f"render_compressed against the decoded render: max difference {err:.3e}")
  assert err <= 1e-5
  colours = scene.colours(cam.camera_position)
  assert bool((colours == 0).any()) and bool((colours == 1).any()) and bool(((colours > 0) & (colours < 1)).any())

  scene.dc.requires_grad_(True)
  scene.sh_codebook.requires_grad_(True)
  view = scene.view(cam.camera_position)
  for name in ('position', 'log_scaling', 'rotation', 'alpha_logit'):
    assert getattr(view, name).data_ptr() == getattr(scene, name).data_ptr(), name
  assert view.feature.shape == (2000, 3)
  view.feature.retain_grad()
  rendered = render_gaussians(view, cam, config, use_sh=False).image
  assert float((rendered.detach() - image).abs().max()) <= 1e-6        # render_compressed is this call
  w = torch.rand(rendered.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
  (rendered * w).sum().backward()
  g_feature = view.feature.grad
  assert g_feature is not None and float(g_feature.abs().max()) > 0
  want = oracle.reference(scene.dc, scene.sh_index, scene.sh_codebook, scene.position, cam.camera_position, g_feature)
  assert float((view.feature.detach().double().cpu() - want['out']).abs().max()) <= 1e-5
  check_gradients(view.feature.detach(), scene.dc.grad, scene.sh_codebook.grad, want, scene.sh_index)

  plan = scene._coded_plan
  scene.colours(cam.camera_position)
  assert scene._coded_plan is plan                          # kept while sh_index is the same tensor
  scene.sh_index = scene.sh_index.clone()
  scene.colours(cam.camera_position)
  assert scene._coded_plan is not plan and scene._coded_plan.index is scene.sh_index


def test_errors_come_before_any_launch():
  _, _, gpu = case(257, 7, 3)
  args = lambda **kw: [kw.get(name, gpu[name]) for name in ('dc', 'index', 'codebook', 'positions', 'cam')]
  with pytest.raises(NotImplementedError, match="camera_pos"):
    evaluate_sh_coded(*args(cam=gpu['cam'].clone().requires_grad_(True)))
  with pytest.raises(ValueError, match="float32"):
    evaluate_sh_coded(*[t.double() if t.is_floating_point() else t for t in args()])
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    evaluate_sh_coded(*[t.cpu() for t in args()])
  with pytest.raises(ValueError, match="another sh_index"):
    evaluate_sh_coded(*args(), plan=make_coded_sh_plan(gpu['index'].clone(), 7))
  scene, cam = renderer_scene()
  with pytest.raises(ValueError, match="use_sh"):
    render_compressed(scene, cam, use_sh=True)
  with pytest.raises(ValueError, match="sh_degree"):
    render_compressed(scene, cam, sh_degree=2)


def test_finetune_example_lowers_the_loss():
  """a fresh child process: 50 Adam steps on dc and sh_codebook through render_compressed.  The image is linear in the
  colours, so the MSE is convex in both: the loss must go down (a condition, not a measured ratio)."""
  done = subprocess.run([sys.executable, '-m', 'taichi_splatting_amd.examples.finetune_compressed', '--n', '2000', '--codes', '8',
                         '--cameras', '2', '--steps', '50', '--lr', '1e-3', '--size', '160', '96'],
                        capture_output=True, text=True, timeout=120, cwd=str(ROOT))
  assert done.returncode == 0, done.stderr[-2000:]
  report = json.loads(done.stdout.strip().splitlines()[-1])
  print(report)
  assert report['steps'] == 50 and report['final_loss'] < report['initial_loss']
  assert report['psnr_after_db'] > report['psnr_before_db']


def test_render_scene_tool_renders_from_the_codebook(tmp_path):
  """``tools/render_scene.py scene.ply --sh-codes 16 --coded`` in a child process: the coded render against the decoded
  one is at least 80 dB (a 1e-4 RMS difference at peak 1), and both frame times are reported"""
  torch.manual_seed(8)
  cam = random_camera(image_size=(160, 96))
  g = random_3d_gaussians(300, cam).replace(feature=(torch.rand(300, 3, 9) - 0.5) * 0.5)
  save_ply(g, tmp_path / 'scene.ply')
  tool = str(ROOT / 'tools' / 'render_scene.py')
  done = subprocess.run([sys.executable, tool, str(tmp_path / 'scene.ply'), '--sh-codes', '16', '--coded', '--views', '2',
                         '--size', '64', '48'], capture_output=True, text=True, timeout=120)
  assert done.returncode == 0, done.stderr[-2000:]
  q = json.loads(done.stdout.strip().splitlines()[-1])['quantised']
  assert q['sh_codes'] == 16 and q['coded_frame_ms'] > 0 and q['decoded_frame_ms'] > 0
  assert q['coded_psnr_db'] is None or q['coded_psnr_db'] >= 80.0          # None: the renders are identical
  plain = subprocess.run([sys.executable, tool, str(tmp_path / 'scene.ply'), '--sh-codes', '16', '--views', '2', '--size', '64', '48'],
                         capture_output=True, text=True, timeout=120)
  assert plain.returncode == 0, plain.stderr[-2000:]
  assert not any(key.startswith('coded') for key in json.loads(plain.stdout.strip().splitlines()[-1])['quantised'])
