"""CPU tests of the host-side pieces added in round 3: reference module paths kept importable, strip balancing with
rows the mapper culls."""
import torch

import taichi_splatting_amd as pkg
from taichi_splatting_amd import RasterConfig


def test_reference_module_paths_stay_importable():
  pkg.install_as_taichi_splatting()
  from taichi_splatting.optim.util import (get_vector_state, get_scalar_state, get_total_weight, get_running_vis,
                                           flatten_param)
  from taichi_splatting.benchmarks.util import benchmarked            # noqa: F401
  import taichi_splatting.benchmarks.bench_projection as bp
  import taichi_splatting.benchmarks.bench_rasterizer as br
  import taichi_splatting.benchmarks.bench_tilemapper as bt
  import taichi_splatting.benchmarks.bench_sh as bs
  assert all(callable(m.main) for m in (bp, br, bt, bs))
  p = torch.zeros(5, 2, 3, requires_grad=True)
  state = {}
  first, second = get_vector_state(state, p)
  assert first.shape == (5, 6) and second.shape == (5,) and state['v'] is first and state['m'] is second
  first, second = get_scalar_state({}, p)
  assert first.shape == (5, 6) and second.shape == (5, 6)
  assert get_total_weight(state, 5, p.device).shape == (5,) and get_running_vis(state, (5,), p.device).shape == (5,)
  p.grad = torch.ones_like(p)
  flat, grad = flatten_param(p)
  assert flat.shape == (5, 6) and grad.shape == (5, 6)


def test_overlap_balanced_bounds_ignores_rows_the_mapper_culls():
  # alpha below the threshold / NaN / inf rows made NaN tile indexes (INT64_MIN after the cast)
  from taichi_splatting_amd.distributed import overlap_balanced_bounds
  torch.manual_seed(0)
  g = torch.rand(400, 7)
  g[:, 0:2] *= 256
  g[:, 4:6] += 1.0
  g[:, 6] = 0.5
  clean = overlap_balanced_bounds(g, (256, 256), RasterConfig(), 4)
  dirty = g.clone()
  extra = g[:6].clone()
  extra[0, 6] = 1e-4; extra[1, 6] = float('nan'); extra[2, 4] = float('inf'); extra[3, 1] = float('nan')
  extra[4, 6] = 0.0; extra[5, 5] = float('-inf')
  assert overlap_balanced_bounds(torch.cat([dirty, extra]), (256, 256), RasterConfig(), 4) == clean
  assert clean[0] == 0 and clean[-1] == 16 and all(b1 >= b0 for b0, b1 in zip(clean, clean[1:]))
