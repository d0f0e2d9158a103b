"""-m gpu: the gaussian-sharded / strip-sharded renderer (distributed.render_sharded_step) with REAL
processes: ``world`` ranks share the one GPU of the box, process group = gloo, the all-to-all staged
through host memory (all_to_all_via_host).  Every rank holds only its shard of the gaussians; its strip
and the gradients of its shard must equal the single-process full-frame render."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _free_port():
  s = socket.socket()
  s.bind(('127.0.0.1', 0))
  port = s.getsockname()[1]
  s.close()
  return port


def _worker(rank, world, port, dtype_name, balance, ret):
  os.environ['MASTER_ADDR'] = '127.0.0.1'
  os.environ['MASTER_PORT'] = str(port)
  dist.init_process_group('gloo', rank=rank, world_size=world)
  try:
    from taichi_splatting_amd import RasterConfig, render_gaussians
    from taichi_splatting_amd.distributed import (render_sharded_step, shard_range, strip_bounds,
                                                  all_to_all_via_host)
    from taichi_splatting_amd.testing import random_camera, random_3d_gaussians
    dtype = getattr(torch, dtype_name)
    torch.manual_seed(world)           # same scene on every rank; each keeps its shard
    size = (320, 208)
    cam = random_camera(image_size=size)
    n = 20000
    g = random_3d_gaussians(n, cam, scale_factor=1.5, alpha_range=(0.1, 0.9))
    g = g.replace(feature=(torch.rand(n, 3, 16) - 0.5) * 0.5).to(dtype=dtype)
    cam = cam.to(device=DEV, dtype=dtype)
    cfg = RasterConfig(compute_visibility=True, compute_point_heuristic=True)
    torch.manual_seed(0)
    G = torch.randn(size[1], size[0], 3, dtype=dtype, device=DEV)

    tiles_high = (size[1] + 15) // 16
    bounds = strip_bounds(tiles_high, world, [1.0 + (r % 3) for r in range(tiles_high)] if balance else None)
    b, e = shard_range(n, world, rank)
    shard = g[b:e].to(DEV).requires_grad_(True)
    rendering, _ = render_sharded_step(shard, cam, cfg, lambda img, px: (img * G[px[0]:px[1]]).sum(), use_sh=True,
                                       rank=rank, world_size=world, index_offset=b, bounds=bounds,
                                       exchange=all_to_all_via_host, point_stats=(stats := {}))

    full = g.to(DEV).requires_grad_(True)
    r = render_gaussians(full, cam, cfg, use_sh=True)
    (r.image * G).sum().backward()

    y0, y1 = bounds[rank] * 16, min(bounds[rank + 1] * 16, size[1])
    tol = 1e-10 if dtype == torch.float64 else 1e-5
    ok = rendering.image.shape[0] == y1 - y0 and torch.allclose(rendering.image, r.image[y0:y1], atol=tol)
    ok = ok and torch.allclose(rendering.image_weight, r.image_weight[y0:y1], atol=tol)
    ids = rendering.points.idx
    ok = ok and bool((ids[1:] > ids[:-1]).all()) and int(ids.min()) >= 0 and int(ids.max()) < n
    worst = 0.0
    # render_sharded_step is the MODULAR composition (rasterizer -> d axis, d sigma -> exchange -> projection backward,
    # the reference's structure); the full frame hands the projection backward a covariance gradient.  In float32 the
    # modular chain loses digits on the few gaussians whose projected covariance is nearly isotropic (the axis gradient
    # is a small perpendicular component next to a large parallel one; tests/test_gpu_frame.py::assert_grads_close), so
    # the three leaves behind the projection backward are compared on 99 % of the rows there; float64 on every row.
    # (The sync-free steps of sharded.py exchange covariance gradients and are held to the maximum:
    # tests/test_gpu_sharded_static.py.)
    for k, (got, want) in enumerate(zip(
        [shard.position.grad, shard.log_scaling.grad, shard.rotation.grad, shard.alpha_logit.grad, shard.feature.grad],
        [full.position.grad, full.log_scaling.grad, full.rotation.grad, full.alpha_logit.grad, full.feature.grad])):
      want = want[b:e]
      scale = max(1.0, want.abs().max().item())
      rows = (got - want).abs().reshape(got.shape[0], -1).max(dim=1).values
      if dtype == torch.float32 and k < 3 and rows.numel() > 200:
        err = (rows.float().kthvalue(int(rows.numel() * 0.99))[0] / scale).item()
      else:
        err = (rows.max() / scale).item()
      worst = max(worst, err)
      ok = ok and err < (1e-8 if dtype == torch.float64 else 2e-3)
    # visibility / split heuristics of the OWNED gaussians, summed over the strips and sent home
    vis_full = torch.zeros(n, dtype=dtype, device=DEV); vis_full[r.points.idx] = r.points.visibility
    heur_full = torch.zeros(n, 2, dtype=dtype, device=DEV)
    heur_full[r.points.idx] = torch.stack([r.points.prune_cost, r.points.split_score], dim=1)
    stol = dict(rtol=1e-6, atol=1e-9) if dtype == torch.float64 else dict(rtol=2e-3, atol=1e-4 * float(heur_full.abs().max()))
    ok = ok and torch.allclose(stats['visibility'], vis_full[b:e], rtol=stol['rtol'], atol=1e-5 if dtype == torch.float32 else 1e-9)
    ok = ok and torch.allclose(stats['point_heuristic'], heur_full[b:e], **stol) and float(vis_full[b:e].sum()) > 0
    ret[rank] = (bool(ok), worst)
  finally:
    dist.destroy_process_group()


@pytest.mark.parametrize('world,bounds', [(1, [0, 13]), (2, [0, 6, 13]), (5, [0, 4, 4, 9, 12, 13]), (8, None), (64, None)])
def test_routing_kernels_match_torch_formulation(world, bounds):
  # csrc/strip_route.hip against the torch formulation of the same split: identical send buffer
  # (bit-exact rows, order, split sizes) and identical gradient return path
  from taichi_splatting_amd import RasterConfig
  from taichi_splatting_amd import distributed as D
  from taichi_splatting_amd.misc.renderer2d import project_gaussians2d
  from taichi_splatting_amd.testing import random_2d_gaussians
  torch.manual_seed(world)
  size = (300, 13 * 16 - 5) if bounds is not None else (256, 1024)
  n = 50000
  g = random_2d_gaussians(n, size, scale_factor=2.0, alpha_range=(0.0, 0.9)).to(DEV)      # some alphas below the threshold
  p = project_gaussians2d(g)
  p[::97, 1] = float('nan'); p[5::101, 4] = float('inf'); p[7::89, 1] = -500.0; p[11::83, 1] = 1e6
  cfg = RasterConfig()
  tiles_high = (size[1] + 15) // 16
  if bounds is None:
    bounds = D.strip_bounds(tiles_high, world)
  ids = torch.randperm(n, device=DEV)

  def loopback(send, send_counts, recv_counts, group):
    return send.clone()

  out = {}
  for force in (False, True):
    D.FORCE_TORCH_ROUTING = force
    try:
      pp = p.clone().requires_grad_(True); ff = g.feature.clone().requires_grad_(True)
      g2, f2, d, gid = D.exchange_to_strips(pp, ff, g.depths, size, cfg, bounds, global_index=ids, index_offset=1000,
                                            exchange=loopback)
      torch.manual_seed(1)
      (g2 * torch.randn_like(g2)).sum().backward(retain_graph=True)
      (f2 * torch.randn_like(f2)).sum().backward()
      out[force] = (g2.detach(), f2.detach(), d, gid, pp.grad, ff.grad)
    finally:
      D.FORCE_TORCH_ROUTING = False
  assert out[False][0].shape[0] > n // 2
  for k, (a, b) in enumerate(zip(out[False], out[True])):
    a, b = torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)
    assert a.shape == b.shape
    if k < 4:
      assert torch.equal(a, b), k
    else:      # sums over the copies of a splat: atomics, order not fixed
      assert torch.allclose(a, b, rtol=1e-5, atol=1e-5), k


@pytest.mark.parametrize('world,capacity_frac', [(1, None), (3, None), (8, None), (8, 0.6)])
def test_return_rows_and_slot_table_match_return_grads(world, capacity_frac):
  """ms_strip_route_pack_slots / ms_strip_return_rows (interleaved home rows) / the slot-table gather against
  ms_strip_route_pack + ms_strip_return_grads: same send buffer, same per-splat gradient sums; with buckets too small
  for the splats (capacity_frac) the dropped copies carry slot -1 and contribute nothing anywhere"""
  import ctypes
  from taichi_splatting_amd import RasterConfig, _lib
  from taichi_splatting_amd import distributed as D
  from taichi_splatting_amd.misc.renderer2d import project_gaussians2d
  from taichi_splatting_amd.testing import random_2d_gaussians
  lib = _lib.load()
  torch.manual_seed(world)
  size, n, f = (256, 512), 30000, 3
  g = random_2d_gaussians(n, size, scale_factor=3.0, alpha_range=(0.05, 0.9)).to(DEV)
  p = project_gaussians2d(g).contiguous()
  feats, depth = g.feature.contiguous(), g.depths.reshape(-1).contiguous()
  cfg = RasterConfig()
  bounds = D.strip_bounds((size[1] + 15) // 16, world)
  stream = _lib.current_stream(p.device)
  nb = lib.ms_strip_route_blocks(n)
  route = torch.empty((n,), dtype=torch.int32, device=DEV)
  block_offsets = torch.empty((world * nb,), dtype=torch.int32, device=DEV)
  send_counts = torch.empty((world,), dtype=torch.int64, device=DEV)
  bounds_c = (ctypes.c_int32 * (world + 1))(*bounds)
  _lib.check(lib.ms_strip_route_count(p.data_ptr(), depth.data_ptr(), n, size[1], cfg.tile_size, cfg.alpha_threshold,
                                      ctypes.cast(bounds_c, ctypes.c_void_p), world, route.data_ptr(),
                                      block_offsets.data_ptr(), send_counts.data_ptr(), stream), 'count')
  biggest = int(send_counts.max())
  cap = biggest if capacity_frac is None else max(int(biggest * capacity_frac), 1)
  m, width = world * cap, 9 + f
  flag = torch.zeros((2,), dtype=torch.int32, device=DEV)

  def pack(with_slots):
    send = torch.zeros((m, width), device=DEV)
    send_index = torch.full((m,), -1, dtype=torch.int64, device=DEV)
    slots = torch.full((n, world), -7, dtype=torch.int32, device=DEV)
    if with_slots:
      _lib.check(lib.ms_strip_route_pack_slots(p.data_ptr(), feats.data_ptr(), depth.data_ptr(), None, f, n, world, 0,
                                               route.data_ptr(), block_offsets.data_ptr(), send_counts.data_ptr(), cap,
                                               flag.data_ptr(), send.data_ptr(), send_index.data_ptr(), slots.data_ptr(),
                                               stream), 'pack_slots')
    else:
      _lib.check(lib.ms_strip_route_pack(p.data_ptr(), feats.data_ptr(), depth.data_ptr(), None, f, n, world, 0,
                                         route.data_ptr(), block_offsets.data_ptr(), send_counts.data_ptr(), cap,
                                         flag.data_ptr(), send.data_ptr(), send_index.data_ptr(), stream), 'pack')
    return send, send_index, slots

  send_a, index_a, _ = pack(False)
  send_b, index_b, slots = pack(True)
  assert torch.equal(send_a, send_b) and torch.equal(index_a, index_b)
  assert bool(flag[0]) == (capacity_frac is not None)

  # the slot table: copy c of splat i sits in row slots[i, c] of the send buffer (or was dropped)
  copies = (route >> 16).long()
  for c in range(int(copies.max())):
    has = copies > c
    sl = slots[has, c].long()
    kept = sl >= 0
    assert torch.equal(index_b[sl[kept]], torch.nonzero(has).reshape(-1)[kept])
  assert int((slots[:, 0][copies > 0] >= 0).sum()) + int((slots[:, 1:] >= 0).sum() if world > 1 else 0) == int((index_b >= 0).sum())

  back = torch.randn((m, 7 + f), device=DEV)
  gp, gf = torch.zeros((n, 7), device=DEV), torch.zeros((n, f), device=DEV)
  _lib.check(lib.ms_strip_return_grads(back.data_ptr(), index_b.data_ptr(), route.data_ptr(), f, m, gp.data_ptr(),
                                       gf.data_ptr(), stream), 'return_grads')
  home = torch.zeros((n, 7 + f), device=DEV)
  _lib.check(lib.ms_strip_return_rows(back.data_ptr(), index_b.data_ptr(), route.data_ptr(), f, m, home.data_ptr(), stream),
             'return_rows')
  want = torch.cat([gp, gf], dim=1)
  assert torch.allclose(home, want, rtol=1e-5, atol=1e-5)
  # the gather the per-gaussian pass does (gaussian_bwd.hip, gather_world > 0), restated in torch
  gathered = torch.zeros((n, 7 + f), device=DEV)
  for c in range(world):
    sl = slots[:, c].long()
    use = (copies > c) & (sl >= 0)
    gathered[use] += back[sl[use]]
  assert torch.allclose(gathered, want, rtol=1e-5, atol=1e-5)


_ROUNDS_SIZE, _ROUNDS_MAX_N = (256, 512), 2 * 1024 * 256
_rounds_splats = []       # [projected splats, depths] of the largest case, made once; smaller cases take a prefix


@pytest.mark.parametrize('n', [1024 * 256 + 1, _ROUNDS_MAX_N])
@pytest.mark.parametrize('world,bounds', [(1, None), (3, None), (3, [0, 0, 16, 32])])
def test_route_offsets_carry_the_total_across_rounds(world, bounds, n):
  """route_offsets_kernel scans 1024 blocks per round and carries the total into the next one: 1025 blocks (the smallest
  count with a second round) and 2048 (a full last round), against numpy on the returned route words.  The repeated
  bound leaves strip 0 without a tile row: a destination that receives nothing.  Integers: exact."""
  import ctypes
  import numpy as np
  from taichi_splatting_amd import RasterConfig, _lib
  from taichi_splatting_amd import distributed as D
  from taichi_splatting_amd.misc.renderer2d import project_gaussians2d
  from taichi_splatting_amd.testing import random_2d_gaussians
  lib = _lib.load()
  if not _rounds_splats:
    torch.manual_seed(0)
    g = random_2d_gaussians(_ROUNDS_MAX_N, _ROUNDS_SIZE, scale_factor=3.0, alpha_range=(0.05, 0.9)).to(DEV)
    _rounds_splats.extend([project_gaussians2d(g).contiguous(), g.depths.reshape(-1).contiguous()])
  p, depth = _rounds_splats[0][:n], _rounds_splats[1][:n]
  cfg = RasterConfig()
  tiles_high = (_ROUNDS_SIZE[1] + 15) // 16
  if bounds is None:
    bounds = D.strip_bounds(tiles_high, world)
  nb = lib.ms_strip_route_blocks(n)
  assert nb == (n + 255) // 256 and nb > 1024
  route = torch.empty((n,), dtype=torch.int32, device=DEV)
  block_offsets = torch.full((world * nb,), -1, dtype=torch.int32, device=DEV)
  send_counts = torch.full((world,), -1, dtype=torch.int64, device=DEV)
  bounds_c = (ctypes.c_int32 * (world + 1))(*bounds)
  _lib.check(lib.ms_strip_route_count(p.data_ptr(), depth.data_ptr(), n, _ROUNDS_SIZE[1], cfg.tile_size, cfg.alpha_threshold,
                                      ctypes.cast(bounds_c, ctypes.c_void_p), world, route.data_ptr(),
                                      block_offsets.data_ptr(), send_counts.data_ptr(), _lib.current_stream(p.device)), 'count')
  word = route.cpu().numpy()
  first, copies = (word & 0xffff).astype(np.int64), (word >> 16).astype(np.int64)
  got_offsets, got_counts = block_offsets.cpu().numpy().reshape(world, nb), send_counts.cpu().numpy()
  for d in range(world):
    routed = np.zeros((nb * 256,), dtype=np.int64)
    routed[:n] = (first <= d) & (d < first + copies)
    per_block = routed.reshape(nb, 256).sum(axis=1)
    assert np.array_equal(got_offsets[d], np.cumsum(per_block) - per_block), d
    assert got_counts[d] == per_block.sum(), d
  assert got_counts.sum() > n // 2
  if bounds[0] == bounds[1]:
    assert got_counts[0] == 0 and (got_counts[1:] > 0).all()
  else:
    assert (got_counts > 0).all()


@pytest.mark.parametrize('world,dtype_name,balance', [(2, 'float64', False), (3, 'float64', True), (4, 'float32', False),
                                                      (3, 'float32', True), (8, 'float32', False)])
def test_sharded_step_matches_full_frame(world, dtype_name, balance):
  port = _free_port()
  mgr = mp.Manager()
  ret = mgr.dict()
  mp.spawn(_worker, args=(world, port, dtype_name, balance, ret), nprocs=world, join=True)
  assert all(v[0] for v in dict(ret).values()) and len(ret) == world, dict(ret)
