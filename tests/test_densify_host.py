"""Densification (csrc/densify.hip, optim/densify.py), the part that needs no GPU: the C-ABI surface, the argument
checks that come before any launch, the compiler's resources of the move kernel and the torch path CPU tensors take."""
import ctypes
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from taichi_splatting_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / 'include' / 'mi355_splat.h'
DENSIFY = {'ms_densify_plan', 'ms_densify_table', 'ms_densify_move', 'ms_densify_split2d', 'ms_densify_split3d'}


def declared_functions():
  text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
  return set(re.findall(r'\b(ms_[a-z0-9_]+)\s*\(', text))


def test_header_library_and_binding_agree(lib):
  declared = declared_functions()
  assert DENSIFY <= declared, DENSIFY - declared
  for name in DENSIFY:
    assert hasattr(lib, name), f"{name} is not exported"
  assert set(_lib.SIGNATURES) == declared
  # additive only: the ABI generation is unchanged
  assert lib.ms_version() == 501 == _lib.ABI_VERSION
  import taichi_splatting_amd
  assert taichi_splatting_amd.__version__ == '0.5.1'


def test_descriptor_layout_matches_the_header(tmp_path):
  src = tmp_path / 'sizes.c'
  src.write_text("""
    #include <stdio.h>
    #include <stddef.h>
    #include "mi355_splat.h"
    int main(void) {
      printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(ms_densify_array), offsetof(ms_densify_array, child_fill),
             offsetof(ms_densify_array, src), offsetof(ms_densify_array, dst), offsetof(ms_densify_array, row_bytes),
             sizeof(ms_optim_group));
      return 0;
    }
  """)
  exe = tmp_path / 'sizes'
  subprocess.run(['gcc', '-std=c99', '-I', str(HEADER.parent), str(src), '-o', str(exe)], check=True)
  size, o_fill, o_src, o_dst, o_bytes, optim_group = map(int, subprocess.run([str(exe)], check=True, capture_output=True,
                                                                              text=True).stdout.split())
  C = _lib.DensifyArrayC
  assert (ctypes.sizeof(C), C.child_fill.offset, C.src.offset, C.dst.offset, C.row_bytes.offset) == (size, o_fill, o_src, o_dst, o_bytes)
  assert ctypes.sizeof(_lib.OptimGroupC) == optim_group          # no existing struct changed size


def array(row_bytes=16, src=256, dst=512, child_fill=0, struct_size=None):
  a = _lib.DensifyArrayC(struct_size=ctypes.sizeof(_lib.DensifyArrayC) if struct_size is None else struct_size,
                         child_fill=child_fill, src=src, dst=dst, row_bytes=row_bytes)
  return (_lib.DensifyArrayC * 1)(a)


def test_argument_errors_are_reported_without_a_gpu(lib):
  """Every check comes before the first launch (the pointers below are never dereferenced)."""
  err = lambda: lib.ms_last_error_string()
  nbytes = ctypes.c_size_t(0)
  # plan
  assert lib.ms_densify_plan(None, None, 1000, 2, None, None, None, None, ctypes.byref(nbytes), None) == 0 and nbytes.value > 0
  assert lib.ms_densify_plan(None, None, 1000, 0, None, None, None, None, ctypes.byref(nbytes), None) == -1
  assert b'children' in err()
  assert lib.ms_densify_plan(None, None, -1, 2, None, None, None, None, ctypes.byref(nbytes), None) == -1
  assert lib.ms_densify_plan(None, None, 1 << 30, 2, None, None, None, None, ctypes.byref(nbytes), None) == -1
  assert b'int32' in err()
  assert lib.ms_densify_plan(None, None, 1000, 2, None, None, None, None, None, None) == -1
  assert lib.ms_densify_plan(256, 256, 1000, 2, None, 256, None, 256, ctypes.byref(nbytes), None) == -1     # scan is null
  assert b'null' in err()
  assert lib.ms_densify_plan(None, 256, 1000, 2, 256, 256, None, 256, ctypes.byref(nbytes), None) == -1     # mask is null
  # table
  assert lib.ms_densify_table(256, 1000, 0, 10, 256, 256, None) == -1 and b'children' in err()
  assert lib.ms_densify_table(256, 1000, 2, -1, 256, 256, None) == -1 and b'n_out' in err()
  assert lib.ms_densify_table(256, 1000, 2, 3001, 256, 256, None) == -1
  assert lib.ms_densify_table(None, 1000, 2, 10, 256, 256, None) == -1 and b'null' in err()
  assert lib.ms_densify_table(256, 1000, 2, 10, None, 256, None) == -1
  # move
  assert lib.ms_densify_move(array(struct_size=24), 1, 256, 256, 10, 10, None) == -4 and b'ABI' in err()
  assert lib.ms_densify_move(array(struct_size=0), 1, 256, 256, 10, 10, None) == -4
  for bad in (6, 0, -16, (1 << 20) + 4):
    assert lib.ms_densify_move(array(row_bytes=bad), 1, 256, 256, 10, 10, None) == -1, bad
    assert b'row_bytes' in err()
  assert lib.ms_densify_move(array(src=None), 1, 256, 256, 10, 10, None) == -1 and b'null' in err()
  assert lib.ms_densify_move(array(dst=None), 1, 256, 256, 10, 10, None) == -1
  assert lib.ms_densify_move(array(src=258), 1, 256, 256, 10, 10, None) == -1 and b'aligned' in err()
  assert lib.ms_densify_move(array(child_fill=2), 1, 256, 256, 10, 10, None) == -1 and b'child_fill' in err()
  assert lib.ms_densify_move(array(), 1, None, 256, 10, 10, None) == -1 and b'table' in err()
  assert lib.ms_densify_move(array(), 1, 256, None, 10, 10, None) == -1
  assert lib.ms_densify_move(None, 1, 256, 256, 10, 10, None) == -1
  assert lib.ms_densify_move(array(), 1, 256, 256, -1, 10, None) == -1
  assert lib.ms_densify_move(array(), 1, 256, 256, 10, -1, None) == -1
  # a bad descriptor behind a good one is found before anything is launched
  two = (_lib.DensifyArrayC * 2)(array()[0], array(row_bytes=10)[0])
  assert lib.ms_densify_move(two, 2, 256, 256, 10, 10, None) == -1 and b'array 1' in err()
  # nothing to do: no launch, no error
  assert lib.ms_densify_move(array(), 1, 256, 256, 10, 0, None) == 0
  assert lib.ms_densify_move(None, 0, None, None, 10, 10, None) == 0
  # split
  assert lib.ms_densify_split2d(256, 256, 256, None, 0, 10, 0, 256, None, None, None) == -1 and b'children' in err()
  assert lib.ms_densify_split2d(256, 256, 256, None, 0, 9, 2, 256, None, None, None) == -1 and b'multiple' in err()
  assert lib.ms_densify_split2d(256, 256, 256, None, -1, 10, 2, 256, None, None, None) == -1
  assert lib.ms_densify_split2d(None, 256, 256, None, 0, 10, 2, 256, None, None, None) == -1 and b'null' in err()
  assert lib.ms_densify_split2d(256, 256, 256, None, 0, 10, 2, None, None, None, None) == -1
  assert lib.ms_densify_split2d(256, 256, 256, None, 0, 10, 2, 256, None, 256, None) == -1 and b'depth' in err()
  assert lib.ms_densify_split2d(256, 256, 256, None, 0, 0, 2, 256, None, None, None) == 0
  assert lib.ms_densify_split3d(256, 256, 256, 0, 10, 0, 256, None, None) == -1 and b'children' in err()
  assert lib.ms_densify_split3d(256, 256, 256, 0, 10, 3, 256, None, None) == -1
  assert lib.ms_densify_split3d(256, None, 256, 0, 10, 2, 256, None, None) == -1 and b'null' in err()
  assert lib.ms_densify_split3d(256, 256, None, 0, 10, 2, 256, None, None) == -1
  assert lib.ms_densify_split3d(256, 256, 256, 0, 0, 2, 256, None, None) == 0
  rc = lib.ms_densify_move(array(row_bytes=6), 1, 256, 256, 10, 10, None)
  with pytest.raises(ValueError, match="row_bytes"):
    _lib.check(rc, "densify move")


def test_move_kernel_has_no_scratch():
  """The move kernel streams rows through registers: a spill would put a scratch round trip behind every piece."""
  sys.path.insert(0, str(ROOT / 'tools'))
  import kernel_resources as kr
  table = kr.resources(kr.SRC / 'densify.hip')
  move = [r for name, r in table.items() if 'densify_move_kernel' in name]
  assert len(move) == 1, list(table)
  assert move[0].get('scratch', 0) == 0, move[0]
  assert move[0]['vgpr'] <= 64, move[0]
  for name, r in table.items():
    assert r.get('scratch', 0) == 0, (name, r)


def test_kernels_are_refused_for_cpu_tensors():
  from taichi_splatting_amd.optim import plan_densify
  from taichi_splatting_amd.misc.densify import split_gaussians3d
  from taichi_splatting_amd.testing import random_camera, random_3d_gaussians
  mask = torch.zeros(8, dtype=torch.bool)
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    plan_densify(mask, mask, 2)
  cam = random_camera(image_size=(64, 48))
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    split_gaussians3d(random_3d_gaussians(8, cam), n=2)


def make_params(n):
  from taichi_splatting_amd.optim import ParameterClass
  g = torch.Generator().manual_seed(n)
  tensors = dict(position=torch.randn(n, 3, generator=g), feature=torch.randn(n, 3, 4, generator=g),
                 label=torch.randn(n, 1, generator=g))
  state = dict(position=dict(exp_avg=torch.randn(n, 3, generator=g), exp_avg_sq=torch.rand(n, generator=g),
                             running_vis=torch.rand(n, generator=g)),
               feature=dict(exp_avg=torch.randn(n, 12, generator=g)))
  other = dict(position=dict(step=7))
  return ParameterClass(tensors, dict(position=dict(lr=0.1), feature=dict(lr=0.01, momentum=0.5)),
                        optimizer_state=(state, other), optimizer=torch.optim.SGD, lr=1.0)


def test_cpu_tensors_take_the_torch_path():
  """``ParameterClass.densify`` on CPU tensors is ``params[keep].append_tensors(children)`` with parent copies as
  children: same layout, zero state for the children, prune wins over split."""
  n = 13
  params = make_params(n)
  prune = torch.zeros(n, dtype=torch.bool)
  split = torch.zeros(n, dtype=torch.bool)
  prune[[0, 5, 6]] = True
  split[[2, 6, 12]] = True                      # row 6 carries both flags: pruned
  out = params.densify(prune, split, 3, inherit_state=('running_vis',))
  kept = [1, 3, 4, 7, 8, 9, 10, 11]
  rows = torch.tensor(kept + [2, 2, 2, 12, 12, 12])
  assert out.batch_size[0] == len(rows)
  assert list(out.keys()) == list(params.keys()) and out.parameter_groups == params.parameter_groups
  for k in params.keys():
    assert torch.equal(out.tensors[k].detach(), params.tensors[k].detach()[rows]), k
  state, want = out.tensor_state, params.tensor_state
  for name in want:
    for key, t in want[name].items():
      assert torch.equal(state[name][key][:len(kept)], t[kept]), (name, key)
      child = state[name][key][len(kept):]
      assert torch.equal(child, t[rows[len(kept):]] if key == 'running_vis' else torch.zeros_like(child)), (name, key)
  assert out.other_state == params.other_state and out.other_state['position'] == dict(step=7)
  # identity, every row split, replaced children, nothing left
  none = torch.zeros(n, dtype=torch.bool)
  same = params.densify(none, none, 2)
  assert all(torch.equal(same.tensors[k].detach(), params.tensors[k].detach()) for k in params.keys())
  every = params.densify(none, ~none, 2)
  assert torch.equal(every.tensors['position'].detach(), params.tensors['position'].detach().repeat_interleave(2, 0))
  given = params.densify(prune, split, 3, child_tensors=dict(label=torch.arange(6.0).reshape(6, 1)))
  assert torch.equal(given.tensors['label'][len(kept):], torch.arange(6.0).reshape(6, 1))
  with pytest.raises(ValueError, match="no rows left"):
    params.densify(~none, none, 2)
