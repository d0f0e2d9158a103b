"""Vector-quantised scenes: one k-means codebook over the higher SH bands of a scene and a 2-byte index per gaussian
(the scheme of Compact3D, LightGaussian and Niedermayr et al.; the reference package has no counterpart).

45 of the 59 floats of a degree-3 gaussian are the coefficients ``feature[:, :, 1:]``.  ``compress_scene`` clusters those
rows (``misc.kmeans``: assignment on the f32 MFMA, csrc/kmeans.hip) and keeps geometry, opacity and the DC band in
float32 bit for bit: a degree-3 row shrinks from 236 to 58 bytes plus its share of the codebook.  Decoding is plain
torch on purpose (``index_select`` + ``cat``): it runs wherever the tensors are, the CPU included.

File format (``CompressedScene.save`` / ``load_compressed``): an uncompressed ``.npz`` of plain arrays, no pickled
object; the index is stored as ``uint16``.
"""
from __future__ import annotations

from dataclasses import dataclass
import os
from typing import Optional

import numpy as np
import torch

from .data_types import Gaussians3D, RasterConfig

FORMAT_VERSION = 1
_TENSORS = ('position', 'log_scaling', 'rotation', 'alpha_logit', 'dc', 'sh_codebook', 'sh_index')


@dataclass
class CompressedScene:
  position: torch.Tensor      # (N, 3) float32
  log_scaling: torch.Tensor   # (N, 3)
  rotation: torch.Tensor      # (N, 4)
  alpha_logit: torch.Tensor   # (N, 1)
  dc: torch.Tensor            # (N, 3): feature[:, :, 0]
  sh_codebook: torch.Tensor   # (K, 3, M) with M = (sh_degree + 1)^2 - 1: the codes of feature[:, :, 1:]
  sh_index: torch.Tensor      # (N,) int32 into sh_codebook
  sh_degree: int

  def __post_init__(self):
    n, m = self.position.shape[0], (int(self.sh_degree) + 1) ** 2 - 1
    if not 1 <= int(self.sh_degree) <= 3:
      raise ValueError(f"sh_degree must be in 1..3, got {self.sh_degree}")
    want = dict(position=(n, 3), log_scaling=(n, 3), rotation=(n, 4), alpha_logit=(n, 1), dc=(n, 3), sh_index=(n,))
    for name, shape in want.items():
      if tuple(getattr(self, name).shape) != shape:
        raise ValueError(f"{name} must be {shape}, got {tuple(getattr(self, name).shape)}")
    k = self.sh_codebook.shape[0]
    if self.sh_codebook.ndim != 3 or tuple(self.sh_codebook.shape[1:]) != (3, m) or not 1 <= k <= 65536:
      raise ValueError(f"sh_codebook must be (K <= 65536, 3, {m}), got {tuple(self.sh_codebook.shape)}")
    if self.sh_index.dtype != torch.int32:
      raise ValueError(f"sh_index must be int32, got {self.sh_index.dtype}")

  def decode(self, device=None) -> Gaussians3D:
    """The scene as ``Gaussians3D``: ``feature = cat(dc, sh_codebook[sh_index])``, every other field as stored."""
    move = (lambda t: t) if device is None else (lambda t: t.to(device))
    index = move(self.sh_index).long()
    rest = move(self.sh_codebook).index_select(0, index)
    feature = torch.cat([move(self.dc).unsqueeze(2), rest], dim=2)
    return Gaussians3D(position=move(self.position), log_scaling=move(self.log_scaling), rotation=move(self.rotation),
                       alpha_logit=move(self.alpha_logit), feature=feature, batch_size=(self.position.shape[0],))

  @property
  def nbytes(self) -> int:
    """Bytes of the stored form: the float32 fields, the codebook and 2 bytes of index per gaussian."""
    floats = sum(getattr(self, name).numel() for name in _TENSORS if name != 'sh_index')
    return 4 * floats + 2 * self.sh_index.numel()

  def save(self, path) -> None:
    """Write an uncompressed ``.npz`` (``np.savez`` appends ``.npz`` to a name that lacks it)."""
    arrays = {name: getattr(self, name).detach().cpu().numpy() for name in _TENSORS}
    arrays['sh_index'] = arrays['sh_index'].astype(np.uint16)
    np.savez(os.fspath(path), format_version=np.int32(FORMAT_VERSION), sh_degree=np.int32(self.sh_degree), **arrays)

  def colours(self, camera_position: torch.Tensor) -> torch.Tensor:
    """(N, 3) view-dependent colours seen from ``camera_position`` (3,), evaluated from ``dc``, ``sh_codebook`` and
    ``sh_index`` as stored (``spherical_harmonics.evaluate_sh_coded``): nothing is decoded.  Differentiable in ``dc`` and
    ``sh_codebook``.  The summation plan of the backward is kept on the scene and rebuilt when ``sh_index`` is another
    tensor."""
    from .spherical_harmonics import evaluate_sh_coded, make_coded_sh_plan
    plan = getattr(self, '_coded_plan', None)
    if plan is None or plan.index is not self.sh_index or plan.k != self.sh_codebook.shape[0]:
      plan = make_coded_sh_plan(self.sh_index, self.sh_codebook.shape[0])
      self._coded_plan = plan
    return evaluate_sh_coded(self.dc, self.sh_index, self.sh_codebook, self.position.detach(), camera_position, plan=plan)

  def view(self, camera_position: torch.Tensor) -> Gaussians3D:
    """The scene as seen from ``camera_position``: a ``Gaussians3D`` whose ``feature`` is ``colours(camera_position)``
    (plain (N, 3) colours, to be rendered with ``use_sh=False``) and whose other fields are the scene's own tensors."""
    return Gaussians3D(position=self.position, log_scaling=self.log_scaling, rotation=self.rotation,
                       alpha_logit=self.alpha_logit, feature=self.colours(camera_position),
                       batch_size=(self.position.shape[0],))


def load_compressed(path, device='cpu') -> CompressedScene:
  """Read a file written by ``CompressedScene.save``.  ValueError on a file of another layout; pickled objects are
  never loaded."""
  path = os.fspath(path)
  if not os.path.exists(path) and os.path.exists(path + '.npz'):
    path = path + '.npz'
  with np.load(path, allow_pickle=False) as data:
    missing = [name for name in _TENSORS + ('format_version', 'sh_degree') if name not in data.files]
    if missing:
      raise ValueError(f"{path}: not a compressed scene, missing {missing}")
    if int(data['format_version']) != FORMAT_VERSION:
      raise ValueError(f"{path}: format version {int(data['format_version'])}, this reader knows {FORMAT_VERSION}")
    arrays = {name: data[name] for name in _TENSORS}
    degree = int(data['sh_degree'])
  if arrays['sh_index'].dtype != np.uint16:
    raise ValueError(f"{path}: sh_index is {arrays['sh_index'].dtype}, uint16 expected")
  for name in _TENSORS:
    if name != 'sh_index' and arrays[name].dtype != np.float32:
      raise ValueError(f"{path}: {name} is {arrays[name].dtype}, float32 expected")
  tensors = {name: torch.from_numpy(np.ascontiguousarray(a)) for name, a in arrays.items() if name != 'sh_index'}
  tensors['sh_index'] = torch.from_numpy(arrays['sh_index'].astype(np.int32))
  if tensors['sh_index'].numel() and int(tensors['sh_index'].max()) >= tensors['sh_codebook'].shape[0]:
    raise ValueError(f"{path}: an index points past the {tensors['sh_codebook'].shape[0]} codes")
  return CompressedScene(sh_degree=degree, **{name: t.to(device) for name, t in tensors.items()})


def compress_scene(gaussians: Gaussians3D, sh_codes: int = 4096, iterations: int = 10,
                   weights: Optional[torch.Tensor] = None, seed: Optional[int] = None) -> CompressedScene:
  """Vector-quantise the higher SH bands of a scene: k-means with ``sh_codes`` codes over the rows of
  ``feature[:, :, 1:].reshape(N, 3 M)`` (D = 9 / 24 / 45 for degree 1 / 2 / 3).  Geometry, opacity and the DC band are
  kept bit for bit.  ``weights`` (N,) float32 >= 0 is an optional importance per gaussian (for instance the view count
  of ``misc.coverage.Coverage``): centroids become weighted means.  ``seed`` fixes the initial codes.

  ValueError on a plain-colour or degree-0 scene (nothing to quantise), on ``sh_codes`` outside 1..min(N, 65536) and on
  non-finite coefficients.  The scene must be float32 and on the GPU (the clustering has no CPU fallback)."""
  from .misc.kmeans import kmeans, MAX_K
  feature = gaussians.feature
  if feature.ndim != 3 or feature.shape[1] != 3:
    raise ValueError(f"compress_scene needs SH features (N, 3, (D + 1)^2), got {tuple(feature.shape)}: nothing to quantise")
  n, bands = feature.shape[0], feature.shape[2]
  degree = int(round(bands ** 0.5)) - 1
  if (degree + 1) ** 2 != bands or not 0 <= degree <= 3:
    raise ValueError(f"SH coefficient count must be 1, 4, 9 or 16, got {bands}")
  if degree == 0:
    raise ValueError("a degree-0 scene has only its DC band: nothing to quantise")
  if not isinstance(sh_codes, int) or isinstance(sh_codes, bool) or not 1 <= sh_codes <= MAX_K:
    raise ValueError(f"sh_codes must be an integer in 1..{MAX_K}, got {sh_codes!r}")
  if sh_codes > n:
    raise ValueError(f"sh_codes = {sh_codes} needs at least as many gaussians, got {n}")
  for name in ('position', 'log_scaling', 'rotation', 'alpha_logit', 'feature'):
    if getattr(gaussians, name).dtype != torch.float32:
      raise ValueError(f"compress_scene stores float32: {name} is {getattr(gaussians, name).dtype}")

  m = bands - 1
  rows = feature.detach()[:, :, 1:].reshape(n, 3 * m).contiguous()
  result = kmeans(rows, sh_codes, iterations=iterations, weights=weights, seed=seed)
  keep = lambda t: t.detach().clone()
  return CompressedScene(position=keep(gaussians.position), log_scaling=keep(gaussians.log_scaling),
                         rotation=keep(gaussians.rotation), alpha_logit=keep(gaussians.alpha_logit),
                         dc=feature.detach()[:, :, 0].clone(), sh_codebook=result.codebook.reshape(sh_codes, 3, m),
                         sh_index=result.index, sh_degree=degree)


def render_compressed(scene: CompressedScene, camera_params, config: RasterConfig = RasterConfig(), **kwargs):
  """``render_gaussians(scene.view(camera_params.camera_position), camera_params, config, use_sh=False, **kwargs)``: a
  compressed scene rendered, and differentiated in ``dc``, ``sh_codebook`` and the geometry, without decoding it.  The
  colours enter the renderer as plain features, so ``use_sh`` and ``sh_degree`` among the kwargs are a ValueError."""
  from .renderer import render_gaussians
  for name in ('use_sh', 'sh_degree'):
    if name in kwargs:
      raise ValueError(f"render_compressed: {name} is not a choice here (the stored SH degree is evaluated into plain colours)")
  return render_gaussians(scene.view(camera_params.camera_position), camera_params, config, use_sh=False, **kwargs)


__all__ = ['CompressedScene', 'compress_scene', 'load_compressed', 'render_compressed', 'FORMAT_VERSION']
