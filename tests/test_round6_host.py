"""Round 6, CPU: host-side bookkeeping added this round (no kernels run)."""
import ctypes

import pytest
import torch

from taichi_splatting_amd import _lib


def test_sized_structs_take_keywords_only():
  with pytest.raises(AssertionError):
    _lib.FrameDescC(1000)
  d = _lib.FrameDescC(n=5)
  assert d.n == 5 and d.struct_size == ctypes.sizeof(_lib.FrameDescC) and d.abi_version == _lib.ABI_VERSION
  g = _lib.OptimGroupC(d=3)
  assert ctypes.sizeof(g) % 8 == 0


def test_optimiser_step_refuses_cpu_tensors_and_bad_dense_shapes():
  from taichi_splatting_amd.optim import ParameterClass, VisibilityAwareAdam
  n = 10
  params = ParameterClass(dict(position=torch.randn(n, 3)), dict(position=dict(lr=0.1)), optimizer=VisibilityAwareAdam)
  params.position.grad = torch.randn(n, 3)
  with pytest.raises(AssertionError, match="one visibility per point"):
    params.step(indexes=None, visibility=torch.rand(n - 1))
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    params.step(indexes=None, visibility=torch.rand(n))
  with pytest.raises(AssertionError, match="shape mismatch"):
    params.step(indexes=torch.arange(4), visibility=torch.rand(5))
