"""Shared by tests/test_coverage_host.py and tests/test_gpu_camera_coverage.py: the scene and camera set of the coverage
tests (built on the CPU, seeded), and the float64 restatement of ``Gaussians3D.with_filter_3d`` with its margins.

The camera set.  ``random_camera`` draws a uniformly random orientation, so a gaussian in view of ALL of 70 such
cameras does not exist; the set is therefore ``random_camera`` under consecutive seeds from ``CAMERA_SEED`` on, keeping
the seeds whose camera has one anchor point (the position of gaussian ``ANCHOR``) inside its image and between its clip
planes — about one seed in ten.  The first camera is the one the gaussians are scattered around.  Image sizes and clip
planes alternate, so that one set holds two of each.  ``python -m tests.coverage_cases`` prints, from
``oracle/projection.py`` on the CPU, the fractions the GPU test asserts on its own yardstick.
"""
import functools
import math

import torch

from taichi_splatting_amd import CameraParams, Gaussians3D
from taichi_splatting_amd.testing.random_data import random_3d_gaussians, random_camera

F32, F64 = torch.float32, torch.float64

N_MAX, C_MAX = 1000, 70
SCENE_SEED, CAMERA_SEED, POS_SCALE = 4, 1000, 1.0
ANCHOR = 1                                 # gaussian every camera looks at; inside every prefix of two or more gaussians
SIZES = ((160, 120), (96, 136))            # (W, H), alternating
NEARS = (0.1, 0.25)                        # far = 1000 near (random_camera), alternating every third camera
LOW_ALPHA = 0.002                          # below 1 / 255 and below the non-default threshold 0.05
LOW_ALPHA_ROWS = slice(3, None, 10)        # a tenth of the gaussians
BEHIND_ROWS = (5, 17, 40)                  # moved behind the first camera
ZERO_QUAT_ROW = 7


def _sees_point(camera: CameraParams, point: torch.Tensor) -> bool:
  pc = camera.T_camera_world.double() @ torch.cat([point.double(), torch.ones(1, dtype=F64)])
  fx, fy, cx, cy = camera.projection.double().tolist()
  x, y, z = pc[:3].tolist()
  if not 2 * camera.near_plane < z < 0.5 * camera.far_plane:
    return False
  w, h = camera.image_size
  return 0 < fx * x / z + cx < w and 0 < fy * y / z + cy < h


@functools.lru_cache(maxsize=None)
def scene():
  """(Gaussians3D of N_MAX rows, list of C_MAX cameras), float32 on the CPU; shared, never modified.  Every test case
  is a prefix of both: whether camera c sees gaussian i does not depend on the other gaussians or cameras."""
  torch.manual_seed(SCENE_SEED)
  first = random_camera(pos_scale=POS_SCALE, image_size=SIZES[0], near_plane=NEARS[0])
  g = random_3d_gaussians(N_MAX, first, scale_factor=1.0, alpha_range=(0.1, 0.9), margin=0.2)

  alpha_logit = g.alpha_logit.clone()
  alpha_logit[LOW_ALPHA_ROWS] = math.log(LOW_ALPHA / (1 - LOW_ALPHA))
  position = g.position.clone()
  camera_world = torch.inverse(first.T_camera_world)
  for k, row in enumerate(BEHIND_ROWS):      # on the optical axis, 0.5, 1.0, 1.5 behind the centre of projection
    position[row] = camera_world[:3, 3] - 0.5 * (k + 1) * camera_world[:3, 2]
  rotation = g.rotation.clone()
  rotation[ZERO_QUAT_ROW] = 0.0
  g = g.replace(position=position, rotation=rotation, alpha_logit=alpha_logit)

  cameras, seed = [first], CAMERA_SEED
  while len(cameras) < C_MAX:
    k = len(cameras)
    torch.manual_seed(seed)
    seed += 1
    camera = random_camera(pos_scale=POS_SCALE, image_size=SIZES[k % 2], near_plane=NEARS[(k % 3) // 2])
    if _sees_point(camera, g.position[ANCHOR]):
      cameras.append(camera)
    assert seed < CAMERA_SEED + 5000, "the seed scan does not terminate"
  return g, cameras


def case(n: int, num_cameras: int, dtype, device):
  g, cameras = scene()
  return g[:n].to(dtype).to(device), [c.to(device=device, dtype=dtype) for c in cameras[:num_cameras]]


def non_vacuous(bits: torch.Tensor) -> dict:
  """what the GPU test asserts of a yardstick matrix bits (C, n) bool"""
  count = bits.sum(dim=0)
  return dict(fraction=bits.double().mean().item(), unseen=int((count == 0).sum()), by_all=int((count == bits.shape[0]).sum()))


# ---- Gaussians3D.with_filter_3d -----------------------------------------------------------------------------------------

def filter_scene(n, dtype, seed=5):
  """scales in [0.3, 3] (|log| <= 1.1: values of order 1), opacities in [0.01, 0.99], a third of the sigmas exactly 0"""
  gen = torch.Generator().manual_seed(seed)
  log_scaling = (torch.rand(n, 3, generator=gen, dtype=F64) * 2 - 1) * math.log(3.0)
  opacity = 0.01 + 0.98 * torch.rand(n, 1, generator=gen, dtype=F64)
  sigma = torch.rand(n, generator=gen, dtype=F64) * 2.0
  sigma[::3] = 0.0
  g = Gaussians3D(position=torch.randn(n, 3, generator=gen, dtype=F64), log_scaling=log_scaling,
                  rotation=torch.randn(n, 4, generator=gen, dtype=F64), alpha_logit=torch.log(opacity / (1 - opacity)),
                  feature=torch.rand(n, 3, generator=gen, dtype=F64), batch_size=(n,))
  return g.to(dtype), sigma.to(dtype)


def filter_formulas(g, sigma):
  """(s', alpha') in float64 from the stored values, written out independently of the implementation:
  s'^2 = s^2 + sigma^2, alpha' = alpha sqrt(prod s^2 / prod s'^2)"""
  s = torch.exp(g.log_scaling.detach().double().cpu())
  s_new = torch.sqrt(s ** 2 + sigma.detach().double().cpu().unsqueeze(1) ** 2)
  alpha = 1.0 / (1.0 + torch.exp(-g.alpha_logit.detach().double().cpu()))
  return s_new, alpha * torch.sqrt((s ** 2).prod(dim=1, keepdim=True) / (s_new ** 2).prod(dim=1, keepdim=True))


def check_filtered(g, sigma, out, dtype):
  """float64: the stored quantities to 1e-12 relative.  Both dtypes, in the well-conditioned space: exp(log_scaling')
  to 1e-6 relative and sigmoid(alpha_logit') to 1e-6 absolute of the float64 value.  sigma == 0 rows bitwise."""
  s_new, alpha_new = filter_formulas(g, sigma)
  log_scaling, alpha_logit = out.log_scaling.detach().cpu(), out.alpha_logit.detach().cpu()
  assert log_scaling.dtype == dtype and alpha_logit.dtype == dtype
  if dtype == F64:
    logit = torch.log(alpha_new / (1 - alpha_new))
    assert ((log_scaling - torch.log(s_new)).abs() <= 1e-12 * torch.log(s_new).abs().clamp_min(1.0)).all()
    assert ((alpha_logit - logit).abs() <= 1e-12 * logit.abs().clamp_min(1.0)).all()
  scale_error = ((torch.exp(log_scaling.double()) - s_new).abs() / s_new).max().item()
  alpha_error = (torch.sigmoid(alpha_logit.double()) - alpha_new).abs().max().item()
  print(f"with_filter_3d {dtype}: scale {scale_error:.3g} relative, alpha {alpha_error:.3g} absolute")
  assert scale_error <= 1e-6 and alpha_error <= 1e-6
  keep = sigma.detach().cpu() == 0
  assert torch.equal(log_scaling[keep], g.log_scaling.detach().cpu()[keep])
  assert torch.equal(alpha_logit[keep], g.alpha_logit.detach().cpu()[keep])
  assert (log_scaling[~keep] >= g.log_scaling.detach().cpu()[~keep]).all()
  assert (alpha_logit[~keep] <= g.alpha_logit.detach().cpu()[~keep]).all()
  return keep


if __name__ == '__main__':
  from oracle import projection as op
  from taichi_splatting_amd import RasterConfig
  g, cameras = scene()
  for config in (RasterConfig(), RasterConfig(blur_cov=0.0, clamp_margin=0.5, alpha_threshold=0.05)):
    bits = torch.stack([op.project_all(*[t.double() for t in g.shape_tensors()][:3], g.alpha_logit.double().squeeze(1),
                                       c.T_camera_world.double(), c.projection.double(), c.image_size, c.depth_range,
                                       config.blur_cov, config.clamp_margin, config.alpha_threshold)[2] for c in cameras])
    print('full', non_vacuous(bits))
    for n in (63, 64, 65, 255, 256, 257, 1000):
      print(n, 33, non_vacuous(bits[:33, :n]))
    for c in (1, 31, 32, 33, 64, 70):
      print(257, c, non_vacuous(bits[:c, :257]))
