"""Spherical-harmonics colour evaluation at gathered indexes.

Same interface as reference ``indexed_spherical_harmonics.py:166-177`` (``evaluate_sh_at``);
forward/backward kernels in csrc/sh.hip (hand-derived backward instead of Taichi autodiff).

``evaluate_sh_coded`` (no reference counterpart) evaluates the colours of a vector-quantised scene from its DC band,
codebook and indices (csrc/sh_coded.hip), with a reproducible codebook gradient.

``sh_rotation_matrices`` / ``rotate_sh`` (no reference counterpart) rotate the bands of stored coefficients, the SH half
of ``Gaussians3D.transformed`` (csrc/scene_transform.hip).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
import functools
import math
from typing import Optional

import torch

from . import _lib


def check_sh_degree(sh_features):
  assert len(sh_features.shape) == 3, f"SH features must have 3 dimensions, got {sh_features.shape}"
  n_sh = sh_features.shape[2]
  n = int(math.sqrt(n_sh))
  assert n * n == n_sh, f"SH feature count must be square, got {n_sh} ({sh_features.shape})"
  return n - 1


def check_active_degree(active_degree, stored_degree: int, what: str = "active_degree") -> int:
  """The active SH degree of a scene stored at ``stored_degree``: ``None`` is all of it.  Nothing is clamped — a trainer's
  band schedule writes ``min(iteration // 1000, D)`` itself."""
  if active_degree is None:
    return stored_degree
  if not isinstance(active_degree, int) or isinstance(active_degree, bool):
    raise ValueError(f"{what} must be None or an int, got {active_degree!r}")
  if not 0 <= active_degree <= stored_degree:
    raise ValueError(f"{what} must be in 0..{stored_degree} (the degree the features are stored at), got {active_degree}")
  return active_degree


class _SHFunction(torch.autograd.Function):
  """reference indexed_spherical_harmonics.py:138-160"""

  @staticmethod
  def forward(ctx, params, points, indexes, camera_pos, degree, unique_indexes, active):
    lib = _lib.load()
    _lib.require_gpu(params, points, indexes, camera_pos)
    params_c, points_c = params.detach().contiguous(), points.detach().contiguous()
    cam_c = camera_pos.detach().contiguous()
    indexes = indexes.contiguous()
    assert indexes.dtype == torch.int64, f"indexes must be int64, got {indexes.dtype}"
    assert points_c.dtype == params_c.dtype and cam_c.dtype == params_c.dtype, "evaluate_sh_at: dtype mismatch"
    v, f = indexes.shape[0], params_c.shape[1]
    out = torch.empty((v, f), dtype=params_c.dtype, device=params_c.device)
    _lib.check(lib.ms_sh_fwd_active(params_c.data_ptr(), points_c.data_ptr(), indexes.data_ptr(), cam_c.data_ptr(),
                                    v, f, degree, active, out.data_ptr(), _lib.dtype_code(params_c.dtype),
                                    _lib.current_stream(params_c.device)), "evaluate_sh_at")
    ctx.save_for_backward(params_c, points_c, cam_c, out)
    ctx.indexes, ctx.degree, ctx.active, ctx.unique = indexes, degree, active, bool(unique_indexes)
    return out

  @staticmethod
  def backward(ctx, doutput):
    lib = _lib.load()
    params, points, camera_pos, out = ctx.saved_tensors
    need_params, need_points, _, need_cam, _, _, _ = ctx.needs_input_grad
    v, f = ctx.indexes.shape[0], params.shape[1]
    # with unique indexes covering every row (all gaussians visible) the streaming kernel writes the
    # whole gradient (the inactive bands of an active degree as zeros): skip the 4*F*D*N byte zero fill (1.15 GB at
    # 6 M gaussians, RGB degree 3)
    all_rows_written = (ctx.unique and v == params.shape[0] and f <= 4 and need_params
                        and not need_points and not need_cam)
    g_params = (torch.empty_like(params) if all_rows_written else torch.zeros_like(params)) if need_params else None
    g_points = torch.zeros_like(points) if need_points else None
    g_cam = torch.zeros_like(camera_pos) if need_cam else None
    if v > 0 and (need_params or need_points or need_cam):
      doutput = doutput.contiguous()
      _lib.check(lib.ms_sh_bwd_active(params.data_ptr(), points.data_ptr(), ctx.indexes.data_ptr(),
                                      camera_pos.data_ptr(), v, f, ctx.degree, ctx.active, out.data_ptr(),
                                      doutput.data_ptr(), _lib.ptr(g_params), _lib.ptr(g_points), _lib.ptr(g_cam),
                                      int(ctx.unique), _lib.dtype_code(params.dtype),
                                      _lib.current_stream(params.device)),
                 "evaluate_sh_at backward")
    return g_params, g_points, None, g_cam, None, None, None


def evaluate_sh_at(sh_params: torch.Tensor,   # M, K, (degree + 1)^2  (usually K=3, for RGB)
                   positions: torch.Tensor,   # M, 3
                   indexes: torch.Tensor,     # N   (indexes to gaussians) 0 to M
                   camera_pos: torch.Tensor,  # 3
                   unique_indexes: bool = False,  # promise: no repeated index (faster backward)
                   *, active_degree: Optional[int] = None   # evaluate bands 0..active_degree only (None: all stored)
                   ) -> torch.Tensor:         # N, K
  """``active_degree=d``: the colours of ``sh_params[:, :, :(d + 1)**2]``, read in place; the gradient keeps the stored
  shape and is exactly zero in the other coefficients.  ``None`` or the stored degree: every band."""
  degree = check_sh_degree(sh_params)
  assert 0 <= degree <= 3, f"SH degree must be between 0 and 3, got {degree}"
  active = check_active_degree(active_degree, degree)
  return _SHFunction.apply(sh_params, positions, indexes, camera_pos, degree, unique_indexes, active)


# ---- colours of a vector-quantised scene from its stored form (csrc/sh_coded.hip; no reference counterpart) ------------

@dataclass
class CodedSHPlan:
  """The order in which ``ms_sh_coded_bwd`` sums the codebook gradient: a function of ``sh_index`` alone, so one plan
  serves every frame and every step of a fine-tune.  ``index`` is the tensor the plan was built from."""
  index: torch.Tensor         # (N,) int32
  order: torch.Tensor         # (N,) int32: the gaussians listed by code, storage order inside a code (stable)
  rank: torch.Tensor          # (N,) int32: the inverse of order, what the kernels read
  chunk_code: torch.Tensor    # (num_chunks,) int32: the code of each chunk of SH_CODED_CHUNK entries
  chunk_begin: torch.Tensor   # (num_chunks,) int32: its first entry of order
  chunk_off: torch.Tensor     # (K + 1,) int32: the first chunk of each code; chunk_off[K] = num_chunks
  num_chunks: int             # read on the host once, here
  k: int
  _scratch_bytes: dict = field(default_factory=dict, repr=False)      # degree -> bytes of ms_sh_coded_bwd's scratch

  @property
  def n(self) -> int:
    return self.index.shape[0]


def make_coded_sh_plan(sh_index: torch.Tensor, k: int) -> CodedSHPlan:
  """Plain torch on the device of ``sh_index`` (the CPU too): stable sort, bincount, cumsum, repeat_interleave.  One host
  read (the index range and the number of chunks).  ValueError on an index outside 0..k-1 or a dtype other than int32."""
  if not isinstance(sh_index, torch.Tensor) or sh_index.ndim != 1:
    raise ValueError(f"sh_index must be a 1D tensor, got {tuple(getattr(sh_index, 'shape', ()))}")
  if sh_index.dtype != torch.int32:
    raise ValueError(f"sh_index must be int32, got {sh_index.dtype}")
  if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= 65536:
    raise ValueError(f"k must be an integer in 1..65536, got {k!r}")
  n, device, chunk = sh_index.shape[0], sh_index.device, _lib.SH_CODED_CHUNK
  wide = sh_index.detach().long()
  if n > 0:
    lo, hi = (int(v) for v in torch.stack([wide.min(), wide.max()]).tolist())
    if lo < 0 or hi >= k:
      raise ValueError(f"sh_index must lie in 0..{k - 1}, got values in {lo}..{hi}")
  order = torch.sort(wide, stable=True).indices
  counts = torch.bincount(wide, minlength=k)
  chunks_per = (counts + (chunk - 1)) // chunk
  chunk_off = torch.zeros((k + 1,), dtype=torch.int64, device=device)
  torch.cumsum(chunks_per, dim=0, out=chunk_off[1:])
  start = torch.cumsum(counts, dim=0) - counts
  num_chunks = int(chunk_off[k])
  codes = torch.arange(k, device=device)
  chunk_code = torch.repeat_interleave(codes, chunks_per, output_size=num_chunks)
  chunk_begin = start[chunk_code] + (torch.arange(num_chunks, device=device) - chunk_off[chunk_code]) * chunk
  rank = torch.empty((n,), dtype=torch.int64, device=device)
  rank[order] = torch.arange(n, device=device)
  i32 = lambda t: t.to(torch.int32).contiguous()
  return CodedSHPlan(index=sh_index, order=i32(order), rank=i32(rank), chunk_code=i32(chunk_code),
                     chunk_begin=i32(chunk_begin), chunk_off=i32(chunk_off), num_chunks=num_chunks, k=k)


def _coded_bwd_call(plan: CodedSHPlan, degree: int, positions, cam, out, g_out, g_dc, g_codebook):
  """``call(tmp_ptr, size_ref)`` of ms_sh_coded_bwd for the scratch helpers of ``_lib``"""
  lib, stream = _lib.load(), None if out is None else _lib.current_stream(out.device)
  return lambda tmp, size: lib.ms_sh_coded_bwd(
    _lib.ptr(positions), _lib.ptr(cam), _lib.ptr(out), _lib.ptr(g_out), _lib.ptr(plan.rank), _lib.ptr(plan.chunk_begin),
    _lib.ptr(plan.chunk_off), plan.num_chunks, plan.n, plan.k, degree, _lib.ptr(g_dc), _lib.ptr(g_codebook), tmp, size,
    stream)


def _coded_bwd(plan: CodedSHPlan, degree: int, positions, cam, out, g_out, g_dc, g_codebook, tmp, nbytes):
  """The bare call on a block (uint8 tensor or None) and a ``c_size_t`` of the caller's; returns the code."""
  return _coded_bwd_call(plan, degree, positions, cam, out, g_out, g_dc, g_codebook)(_lib.ptr(tmp), ctypes.byref(nbytes))


class _CodedSHFunction(torch.autograd.Function):

  @staticmethod
  def forward(ctx, dc, sh_codebook, positions, camera_pos, plan, degree):
    dc_c, codebook_c = dc.detach().contiguous(), sh_codebook.detach().contiguous()
    points_c, cam_c = positions.detach().contiguous(), camera_pos.detach().contiguous()
    n = dc_c.shape[0]
    out = torch.empty((n, 3), dtype=torch.float32, device=dc_c.device)
    _lib.check(_lib.load().ms_sh_coded_fwd(dc_c.data_ptr(), plan.index.data_ptr(), codebook_c.data_ptr(), points_c.data_ptr(),
                                           cam_c.data_ptr(), n, plan.k, degree, out.data_ptr(),
                                           _lib.current_stream(dc_c.device)), "evaluate_sh_coded")
    ctx.save_for_backward(points_c, cam_c, out)
    ctx.plan, ctx.degree = plan, degree
    ctx.codebook_shape = tuple(codebook_c.shape)
    return out

  @staticmethod
  def backward(ctx, g_out):
    points, cam, out = ctx.saved_tensors
    plan, degree = ctx.plan, ctx.degree
    need_dc, need_codebook = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    if not (need_dc or need_codebook):
      return (None,) * 6
    g_out = g_out.contiguous()
    g_dc = torch.empty_like(out) if need_dc else None
    # every row is written, the rows of codes without members as zeros: no zero fill
    g_codebook = torch.empty(ctx.codebook_shape, dtype=torch.float32, device=out.device) if need_codebook else None
    if degree not in plan._scratch_bytes:
      plan._scratch_bytes[degree] = _lib.scratch_bytes(_coded_bwd_call(plan, degree, None, None, None, None, None, None),
                                                       "evaluate_sh_coded backward")
    _lib.run_in_scratch(_coded_bwd_call(plan, degree, points, cam, out, g_out, g_dc, g_codebook),
                        _lib.scratch_block(plan._scratch_bytes[degree], out.device), "evaluate_sh_coded backward")
    return g_dc, g_codebook, None, None, None, None


def evaluate_sh_coded(dc: torch.Tensor,             # N, 3: the DC band
                      sh_index: torch.Tensor,       # N int32 into sh_codebook
                      sh_codebook: torch.Tensor,    # K, 3, (degree + 1)^2 - 1: the codes of the higher bands
                      positions: torch.Tensor,      # N, 3
                      camera_pos: torch.Tensor,     # 3
                      *, plan: Optional[CodedSHPlan] = None) -> torch.Tensor:   # N, 3
  """The colours ``evaluate_sh_at(cat(dc[:, :, None], sh_codebook[sh_index]), positions, arange(N), camera_pos)`` of a
  vector-quantised scene (``scene_codec.CompressedScene``) without the decoded (N, 3, D) tensor, in storage order.
  Gradients reach ``dc`` (dense) and ``sh_codebook`` (summed per code in float64 in an order fixed by ``sh_index``: no
  atomics, two runs bitwise equal).  None reaches ``positions``, which the renderer detaches for SH as the reference
  does; a ``camera_pos`` that requires grad is a ``NotImplementedError``.  ``plan`` is ``make_coded_sh_plan(sh_index, K)``;
  ``None`` builds one (a sort and a host read: keep the plan while ``sh_index`` stays).  float32 on the GPU only."""
  if camera_pos.requires_grad:
    raise NotImplementedError("evaluate_sh_coded: no gradient with respect to camera_pos (detach it)")
  floats = dict(dc=dc, sh_codebook=sh_codebook, positions=positions, camera_pos=camera_pos)
  for name, t in floats.items():
    if t.dtype != torch.float32:
      raise ValueError(f"evaluate_sh_coded: {name} must be float32, got {t.dtype}")
  if sh_index.dtype != torch.int32:
    raise ValueError(f"evaluate_sh_coded: sh_index must be int32, got {sh_index.dtype}")
  n = dc.shape[0]
  if tuple(dc.shape) != (n, 3) or tuple(positions.shape) != (n, 3) or tuple(sh_index.shape) != (n,) or camera_pos.numel() != 3:
    raise ValueError(f"evaluate_sh_coded: dc (N, 3), sh_index (N,), positions (N, 3), camera_pos (3,) expected, got "
                     f"{tuple(dc.shape)}, {tuple(sh_index.shape)}, {tuple(positions.shape)}, {tuple(camera_pos.shape)}")
  if sh_codebook.ndim != 3 or sh_codebook.shape[1] != 3 or sh_codebook.shape[2] not in (3, 8, 15) or not 1 <= sh_codebook.shape[0] <= 65536:
    raise ValueError(f"evaluate_sh_coded: sh_codebook must be (K <= 65536, 3, 3 | 8 | 15), got {tuple(sh_codebook.shape)}")
  _lib.require_gpu(dc, sh_index, sh_codebook, positions, camera_pos)
  if len({t.device for t in (dc, sh_index, sh_codebook, positions, camera_pos)}) != 1:
    raise ValueError("evaluate_sh_coded: the tensors are on different devices")
  k, degree = sh_codebook.shape[0], {3: 1, 8: 2, 15: 3}[sh_codebook.shape[2]]
  if plan is None:
    plan = make_coded_sh_plan(sh_index, k)
  elif plan.k != k or plan.n != n or plan.order.device != dc.device:
    raise ValueError(f"evaluate_sh_coded: the plan is for N = {plan.n}, K = {plan.k} on {plan.order.device}")
  if plan.index is not sh_index:      # a plan of other indices would still sum every product, under the wrong code
    if plan.index.data_ptr() != sh_index.data_ptr() or plan.index.shape != sh_index.shape:
      raise ValueError("evaluate_sh_coded: the plan was built from another sh_index tensor")
  if not plan.index.is_contiguous():
    raise ValueError("evaluate_sh_coded: sh_index must be contiguous")
  return _CodedSHFunction.apply(dc, sh_codebook, positions, camera_pos, plan, degree)


# ---- rotating the bands: Gaussians3D.transformed / ms_scene_transform (csrc/scene_transform.hip) ------------------------

def _rsh_cart_f64(xyz: torch.Tensor, degree: int) -> torch.Tensor:
  """The real basis of csrc/splat_math.h (``sh_basis``) at unit directions (M, 3), float64 on the host: (M, (degree+1)^2)."""
  x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
  out = [torch.full_like(x, 0.282094791773878)]
  if degree >= 1:
    out += [-0.48860251190292 * y, 0.48860251190292 * z, -0.48860251190292 * x]
  if degree >= 2:
    x2, y2, z2 = x * x, y * y, z * z
    out += [1.09254843059208 * (x * y), -1.09254843059208 * (y * z), 0.94617469575756 * z2 - 0.31539156525252,
            -1.09254843059208 * (x * z), 0.54627421529604 * x2 - 0.54627421529604 * y2]
  if degree >= 3:
    out += [-0.590043589926644 * y * (3.0 * x2 - y2), 2.89061144264055 * (x * y) * z,
            0.304697199642977 * y * (1.5 - 7.5 * z2), 1.24392110863372 * z * (1.5 * z2 - 0.5) - 0.497568443453487 * z,
            0.304697199642977 * x * (1.5 - 7.5 * z2), 1.44530572132028 * z * (x2 - y2),
            -0.590043589926644 * x * (x2 - 3.0 * y2)]
  return torch.stack(out, dim=-1)


@functools.lru_cache(maxsize=None)
def _solve_directions():
  """(D, pinv(Y_1(D)), pinv(Y_2(D)), pinv(Y_3(D))) for 48 fixed unit directions D (a Fibonacci spiral): the band blocks
  of the basis sampled there have condition numbers below 1.05, so the least-squares solve of
  ``sh_rotation_matrices`` loses no digits.  Computed once per process."""
  k = torch.arange(48, dtype=torch.float64) + 0.5
  z = 1.0 - 2.0 * k / 48.0
  phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
  r = torch.sqrt(1.0 - z * z)
  dirs = torch.stack([r * torch.cos(phi), r * torch.sin(phi), z], dim=-1)
  y = _rsh_cart_f64(dirs, 3)
  return (dirs,) + tuple(torch.linalg.pinv(y[:, l * l:(l + 1) * (l + 1)]) for l in (1, 2, 3))


def _mul_sum(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
  """a (I, K) times b (K, J) as products summed in index order: the same bits on every call, which a threaded BLAS or
  LAPACK does not promise (the in-place and out-of-place forms of a transform must agree bit for bit)."""
  out = torch.zeros((a.shape[0], b.shape[1]), dtype=torch.float64)
  for k in range(a.shape[1]):
    out += a[:, k:k + 1] * b[k:k + 1, :]
  return out


def check_rotation(R, what: str = "R") -> torch.Tensor:
  """``R`` as a float64 CPU (3, 3) proper rotation, or ``ValueError``: ``|R^T R - I|_inf <= 1e-5`` and ``det > 0``."""
  if not isinstance(R, torch.Tensor) or R.shape != (3, 3):
    raise ValueError(f"{what} must be a (3, 3) tensor, got {tuple(getattr(R, 'shape', ()))}")
  R = R.detach().to(device='cpu', dtype=torch.float64)
  if not bool(torch.isfinite(R).all()):
    raise ValueError(f"{what} has non-finite entries")
  off = float((R.T @ R - torch.eye(3, dtype=torch.float64)).abs().max())
  if off > 1e-5:
    raise ValueError(f"{what} is not a rotation: |R^T R - I| = {off:.3g} > 1e-5 (shear or non-uniform scale)")
  if not float(torch.linalg.det(R)) > 0:
    raise ValueError(f"{what} is a reflection (det < 0), not a rotation")
  return R


def sh_rotation_matrices(R: torch.Tensor, degree: int) -> list:
  """``[M_0 .. M_degree]``, float64 on the CPU, ``M_l`` of shape (2l+1, 2l+1) with ``Y_l(R d) = M_l Y_l(d)`` for every
  unit ``d`` in the basis of ``evaluate_sh_at`` (band l = coefficients l^2 .. (l+1)^2 - 1).  A scene rotated by ``R``
  keeps its colours when every band of coefficients is replaced by ``M_l c_l``.  ``M_1 = P R P^T`` with
  ``P = [[0,-1,0],[0,0,1],[-1,0,0]]`` (band 1 is k (-y, z, -x)).

  Solved exactly from the basis at a fixed, well-conditioned set of directions: ``M_l = Y_l(R D) pinv(Y_l(D))``."""
  if not isinstance(degree, int) or isinstance(degree, bool) or not 0 <= degree <= 3:
    raise ValueError(f"degree must be an integer in 0..3, got {degree!r}")
  R = check_rotation(R)
  dirs, *pinv = _solve_directions()
  y1 = _rsh_cart_f64(_mul_sum(dirs, R.T), degree)
  out = [torch.ones((1, 1), dtype=torch.float64)]
  for l in range(1, degree + 1):
    # rows are directions: Y_l(R D) = Y_l(D) M^T  =>  M^T = pinv(Y_l(D)) Y_l(R D)
    out.append(_mul_sum(pinv[l - 1], y1[:, l * l:(l + 1) * (l + 1)]).T.contiguous())
  return out


def rotation_to_quat(R: torch.Tensor) -> torch.Tensor:
  """The unit xyzw quaternion of a rotation matrix, float64 on the CPU, with w >= 0: the largest component from the
  diagonal, the other three from the off-diagonal sums and differences divided by it, so that every component is good
  to a few 1e-16 (``data_types._mat_to_quat`` takes four square roots and loses half the digits of a small component)."""
  m = check_rotation(R).tolist()
  four_sq = (1.0 + m[0][0] - m[1][1] - m[2][2], 1.0 - m[0][0] + m[1][1] - m[2][2], 1.0 - m[0][0] - m[1][1] + m[2][2],
             1.0 + m[0][0] + m[1][1] + m[2][2])                                      # 4 x^2, 4 y^2, 4 z^2, 4 w^2
  k = max(range(4), key=lambda i: four_sq[i])
  big = 0.5 * math.sqrt(four_sq[k])
  d = 4.0 * big
  if k == 3:
    q = [(m[2][1] - m[1][2]) / d, (m[0][2] - m[2][0]) / d, (m[1][0] - m[0][1]) / d, big]
  elif k == 0:
    q = [big, (m[0][1] + m[1][0]) / d, (m[0][2] + m[2][0]) / d, (m[2][1] - m[1][2]) / d]
  elif k == 1:
    q = [(m[0][1] + m[1][0]) / d, big, (m[1][2] + m[2][1]) / d, (m[0][2] - m[2][0]) / d]
  else:
    q = [(m[0][2] + m[2][0]) / d, (m[1][2] + m[2][1]) / d, big, (m[1][0] - m[0][1]) / d]
  norm = math.sqrt(sum(c * c for c in q))
  sign = -1.0 if q[3] < 0 else 1.0
  return torch.tensor([sign * c / norm for c in q], dtype=torch.float64)


def pack_scene_transform(s: float, R: torch.Tensor, t: torch.Tensor, degree: int = 3):
  """The host array of ``ms_scene_transform`` (MS_SCENE_XFORM_* of include/mi355_splat.h): ``[s R | t]``, ``ln s``,
  ``q_R`` (xyzw), ``M_1 .. M_degree`` (the matrices above ``degree`` stay zero: the kernel does not read them)."""
  R = check_rotation(R)
  if not (s > 0 and math.isfinite(s)):
    raise ValueError(f"scale must be positive and finite, got {s}")
  t = t.detach().to(device='cpu', dtype=torch.float64).reshape(3)
  values = torch.zeros(_lib.SCENE_XFORM_VALUES, dtype=torch.float64)
  values[:12] = torch.cat([s * R, t.view(3, 1)], dim=1).reshape(12)
  values[12] = math.log(s)
  values[13:17] = rotation_to_quat(R)
  at = 17
  for m in sh_rotation_matrices(R, degree)[1:]:
    values[at:at + m.numel()] = m.reshape(-1)
    at += m.numel()
  return (ctypes.c_double * _lib.SCENE_XFORM_VALUES)(*values.tolist())


def scene_transform(packed, *, position=None, log_scaling=None, rotation=None, feature=None, out_position=None,
                    out_log_scaling=None, out_rotation=None, out_feature=None) -> None:
  """One ``ms_scene_transform`` launch on the current stream: each given field from its tensor into its ``out_`` tensor
  (the same tensor: in place).  ``feature`` is (N, F, (D+1)^2) with D in 1..3.  No host read, no allocation."""
  pairs = ((position, out_position, 3), (log_scaling, out_log_scaling, 3), (rotation, out_rotation, 4), (feature, out_feature, None))
  given = [p for p in pairs if p[0] is not None]
  assert given, "scene_transform: no field given"
  _lib.require_gpu(*[x for p in given for x in p[:2]])
  first = given[0][0]
  n, f, degree = first.shape[0], 1, 0
  for src, dst, width in given:
    assert dst is not None and dst.shape == src.shape and dst.dtype == first.dtype and src.dtype == first.dtype \
      and dst.device == first.device and src.device == first.device, "scene_transform: out tensors must match their inputs"
    assert src.is_contiguous() and dst.is_contiguous(), "scene_transform: contiguous tensors expected"
    assert src.shape[0] == n and (width is None or src.shape[1:] == (width,)), f"scene_transform: unexpected shape {tuple(src.shape)}"
  if feature is not None:
    degree = check_sh_degree(feature)
    f = feature.shape[1]
  p = lambda x: None if x is None else x.data_ptr()
  _lib.check(_lib.load().ms_scene_transform(p(position), p(out_position), p(log_scaling), p(out_log_scaling), p(rotation),
                                            p(out_rotation), p(feature), p(out_feature), n, f, degree,
                                            _lib.dtype_code(first.dtype), packed, _lib.current_stream(first.device)),
             "scene_transform")


def rotate_sh(feature: torch.Tensor, R: torch.Tensor, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
  """The SH coefficients (N, F, (D+1)^2) of a scene rotated by ``R``: every band replaced by ``M_l(R) c_l``
  (``sh_rotation_matrices``), one launch on the GPU.  ``out=feature`` works in place.  A degree-0 feature has nothing
  to rotate: it is returned as it is (``out=None``) or copied into ``out``.  No gradient flows through this call."""
  degree = check_sh_degree(feature)
  assert 0 <= degree <= 3, f"SH degree must be between 0 and 3, got {degree}"
  R = check_rotation(R)
  _lib.require_gpu(feature, out)
  _lib.dtype_code(feature.dtype)
  if out is not None and (out.shape != feature.shape or out.dtype != feature.dtype or out.device != feature.device):
    raise ValueError(f"out must match feature: {tuple(feature.shape)} {feature.dtype} on {feature.device}")
  if degree == 0:
    if out is None:
      return feature
    if out is not feature:
      out.copy_(feature)
    return out
  src = feature.detach()
  src = src if src.is_contiguous() else src.contiguous()
  if out is None:
    out = torch.empty_like(src)
  if not out.is_contiguous():
    raise ValueError("out must be contiguous")
  packed = pack_scene_transform(1.0, R, torch.zeros(3), degree)
  scene_transform(packed, feature=src, out_feature=out.detach())
  return out
