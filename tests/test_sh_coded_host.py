"""The parts of the coded SH path that need no GPU: the summation plan on CPU tensors, the exported names, and the
argument checks of ms_sh_coded_fwd / ms_sh_coded_bwd (they come before any launch)."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import taichi_splatting_amd as tsa
from taichi_splatting_amd import _lib
from taichi_splatting_amd.spherical_harmonics import CodedSHPlan, make_coded_sh_plan

C = _lib.SH_CODED_CHUNK
HEADER = Path(__file__).resolve().parent.parent / 'include' / 'mi355_splat.h'


def interleaved_index(members, seed=0):
  """sh_index with ``members[j]`` gaussians of code j, shuffled into storage order"""
  index = torch.cat([torch.full((m,), j, dtype=torch.int32) for j, m in enumerate(members)])
  return index[torch.randperm(index.shape[0], generator=torch.Generator().manual_seed(seed))].contiguous()


def test_chunk_constant_matches_the_header():
  assert int(re.search(r'#define MS_SH_CODED_CHUNK (\d+)', HEADER.read_text()).group(1)) == C


def test_plan_on_cpu_tensors_is_stable_and_chunks_every_run():
  members = [0, 1, C, C + 1, 0, 3, 2 * C]      # runs of 0, 1, C and C + 1 members (and an empty code between others)
  k = len(members)
  index = interleaved_index(members)
  plan = make_coded_sh_plan(index, k)
  assert isinstance(plan, CodedSHPlan) and plan.k == k and plan.n == sum(members) and plan.index is index
  n = index.shape[0]
  for t in (plan.order, plan.rank, plan.chunk_code, plan.chunk_begin, plan.chunk_off):
    assert t.dtype == torch.int32 and t.device.type == 'cpu' and t.is_contiguous()

  order = plan.order.long()
  assert sorted(order.tolist()) == list(range(n))
  codes = index.long()[order]
  assert bool((codes[1:] >= codes[:-1]).all())                                     # listed by code
  same = codes[1:] == codes[:-1]
  assert bool((order[1:][same] > order[:-1][same]).all())                          # storage order inside a code: stable
  assert torch.equal(plan.rank.long()[order], torch.arange(n))                     # rank is the inverse

  chunks = [(m + C - 1) // C for m in members]
  assert chunks == [0, 1, 1, 2, 0, 1, 2]
  assert plan.num_chunks == sum(chunks) == plan.chunk_code.shape[0] == plan.chunk_begin.shape[0]
  want_off, want_code, want_begin, start = [0], [], [], 0
  for j, m in enumerate(members):
    want_off.append(want_off[-1] + chunks[j])
    for c in range(chunks[j]):
      want_code.append(j)
      want_begin.append(start + c * C)
    start += m
  assert plan.chunk_off.tolist() == want_off
  assert plan.chunk_code.tolist() == want_code
  assert plan.chunk_begin.tolist() == want_begin
  # a chunk ends where the next begins (the last at n) and never holds more than C entries of one code
  ends = plan.chunk_begin.tolist()[1:] + [n]
  for begin, end, code in zip(plan.chunk_begin.tolist(), ends, want_code):
    assert 0 < end - begin <= C and bool((codes[begin:end] == code).all())


def test_plan_of_an_empty_scene_and_of_one_code():
  empty = make_coded_sh_plan(torch.zeros((0,), dtype=torch.int32), 5)
  assert empty.num_chunks == 0 and empty.chunk_off.tolist() == [0] * 6 and empty.order.shape == (0,)
  one = make_coded_sh_plan(torch.zeros((2 * C + 1,), dtype=torch.int32), 1)
  assert one.num_chunks == 3 and one.chunk_begin.tolist() == [0, C, 2 * C] and one.chunk_off.tolist() == [0, 3]
  assert one.order.tolist() == list(range(2 * C + 1))


def test_plan_refuses_bad_indices():
  with pytest.raises(ValueError, match="0..3"):
    make_coded_sh_plan(torch.tensor([0, 4, 1], dtype=torch.int32), 4)
  with pytest.raises(ValueError, match="0..3"):
    make_coded_sh_plan(torch.tensor([0, -1, 1], dtype=torch.int32), 4)
  with pytest.raises(ValueError, match="int32"):
    make_coded_sh_plan(torch.tensor([0, 1, 2], dtype=torch.int64), 4)
  with pytest.raises(ValueError, match="k must be"):
    make_coded_sh_plan(torch.tensor([0], dtype=torch.int32), 0)


def test_new_names_are_exported():
  for name in ('evaluate_sh_coded', 'make_coded_sh_plan', 'CodedSHPlan', 'render_compressed', 'compress_scene'):
    assert name in tsa.__all__ and hasattr(tsa, name), name
  assert hasattr(tsa.CompressedScene, 'colours') and hasattr(tsa.CompressedScene, 'view')
  from taichi_splatting_amd import scene_codec
  assert 'render_compressed' in scene_codec.__all__
  me = tsa.install_as_taichi_splatting()
  import taichi_splatting
  assert taichi_splatting is me and taichi_splatting.render_compressed is tsa.render_compressed
  from taichi_splatting.spherical_harmonics import evaluate_sh_coded
  assert evaluate_sh_coded is tsa.evaluate_sh_coded


def test_operator_refuses_before_any_launch():
  """float64, CPU tensors and a camera that wants a gradient are refused by the Python layer (no GPU needed to see it)"""
  n, k = 4, 2
  dc, pos, cam = torch.zeros((n, 3)), torch.ones((n, 3)), torch.zeros(3)
  index, codebook = torch.zeros((n,), dtype=torch.int32), torch.zeros((k, 3, 15))
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    tsa.evaluate_sh_coded(dc, index, codebook, pos, cam)
  with pytest.raises(ValueError, match="float32"):
    tsa.evaluate_sh_coded(dc.double(), index, codebook.double(), pos.double(), cam.double())
  with pytest.raises(NotImplementedError, match="camera_pos"):
    tsa.evaluate_sh_coded(dc, index, codebook, pos, cam.clone().requires_grad_(True))
  with pytest.raises(ValueError, match="sh_codebook"):
    tsa.evaluate_sh_coded(dc, index, torch.zeros((k, 3, 16)), pos, cam)


def fwd(lib, *, dc=1, index=1, codebook=1, positions=1, cam=1, n=10, k=4, degree=3, out=1):
  return lib.ms_sh_coded_fwd(dc, index, codebook, positions, cam, n, k, degree, out, None)


def bwd(lib, *, positions=1, cam=1, out=1, g_out=1, rank=1, chunk_begin=1, chunk_off=1, num_chunks=1, n=10, k=4, degree=3,
        g_dc=1, g_codebook=1, tmp=1, tmp_bytes=1 << 30):
  nbytes = ctypes.c_size_t(tmp_bytes)
  return lib.ms_sh_coded_bwd(positions, cam, out, g_out, rank, chunk_begin, chunk_off, num_chunks, n, k, degree, g_dc, g_codebook,
                             tmp, ctypes.byref(nbytes), None)


def test_argument_errors_are_reported(lib):
  """MS_ERR_BAD_ARG (-1) before any launch: the pointers below are never dereferenced"""
  for call in (fwd, bwd):
    for bad, word in ((dict(degree=0), b'sh_degree'), (dict(degree=4), b'sh_degree'), (dict(k=0), b'k must'),
                      (dict(k=65537), b'k must'), (dict(n=-1), b'n < 0'), (dict(n=1 << 31), b'2^31')):
      assert call(lib, **bad) == -1, (call.__name__, bad)
      assert word in lib.ms_last_error_string(), (call.__name__, bad, lib.ms_last_error_string())
  for name in ('dc', 'index', 'codebook', 'positions', 'cam', 'out'):
    assert fwd(lib, **{name: None}) == -1
    assert b'null' in lib.ms_last_error_string()
  assert fwd(lib, n=0, dc=None, out=None) == 0                      # nothing to do, nothing launched

  for name in ('positions', 'cam', 'out', 'g_out', 'rank', 'chunk_begin', 'chunk_off'):
    assert bwd(lib, **{name: None}) == -1, name
    assert b'null' in lib.ms_last_error_string()
  assert bwd(lib, num_chunks=11) == -1 and bwd(lib, num_chunks=-1) == -1
  assert lib.ms_sh_coded_bwd(1, 1, 1, 1, 1, 1, 1, 1, 10, 4, 3, 1, 1, 1, None, None) == -1
  assert b'tmp_bytes' in lib.ms_last_error_string()
  assert bwd(lib, tmp_bytes=8) == -3                                 # MS_ERR_TMP_TOO_SMALL
  assert bwd(lib, g_dc=None, g_codebook=None) == 0                   # no gradient wanted: nothing launched


def test_scratch_query(lib):
  """tmp == NULL returns the bytes: the float64 sums of every chunk and a 24-byte record per gaussian"""
  def need(**kw):
    nbytes = ctypes.c_size_t(0)
    args = dict(num_chunks=7, n=3000, k=4, degree=3)
    args.update(kw)
    assert lib.ms_sh_coded_bwd(None, None, None, None, None, None, None, args['num_chunks'], args['n'], args['k'],
                               args['degree'], None, None, None, ctypes.byref(nbytes), None) == 0
    return nbytes.value
  assert 7 * 45 * 8 + 3000 * 24 <= need() < 7 * 45 * 8 + 3000 * 24 + 512
  assert need(degree=1) < need(degree=2) < need() < need(n=3100) and need() < need(num_chunks=8)
  assert need(n=0, num_chunks=0) <= 512
