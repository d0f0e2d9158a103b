"""Float64 reference of ``evaluate_sh_coded`` for tests/test_gpu_sh_coded.py: the decoded rows through the package-independent
``oracle.sh.evaluate_sh_at`` with torch autograd, on the CPU.  Nothing here calls the code under test."""
import math

import torch

from oracle import sh as oracle_sh


def random_case(n, k, degree, seed, index=None):
  """CPU float32 inputs.  The coefficients are scaled so that ``pre = 0.5 + sum_d Y_d p_d`` has a standard deviation of
  about 0.6 (sum_d Y_d^2 = D / 4 pi on the unit sphere): roughly a fifth of the colours clamp at each end."""
  gen = torch.Generator().manual_seed(seed)
  d = (degree + 1) ** 2
  s = 0.6 * math.sqrt(4.0 * math.pi / d)
  if index is None:
    index = torch.randint(0, k, (n,), generator=gen, dtype=torch.int32)
  case = dict(
    degree=degree, k=k, index=index.contiguous(),
    dc=torch.randn((n, 3), generator=gen) * s,
    codebook=torch.randn((k, 3, d - 1), generator=gen) * s,
    positions=torch.randn((n, 3), generator=gen) * 2.0,
    cam=torch.tensor([0.3, -5.0, 0.7]),
    g_out=torch.randn((n, 3), generator=gen))
  # torch.clamp passes the gradient at pre == 0 or 1 and the kernels do not, and a float32 pre within rounding of a
  # corner may fall on its other side: a colour that close (2e-4) has its DC coefficient moved so that pre rises by 1e-3
  pre = unclamped(case['dc'], case['index'], case['codebook'], case['positions'], case['cam'])
  near = torch.minimum(pre.abs(), (pre - 1).abs()) < 2e-4
  case['dc'][near] += 1e-3 / 0.282094791773878
  return case


def unclamped(dc, index, codebook, positions, cam):
  """float64 ``pre = 0.5 + sum_d Y_d p_d`` (N, 3) of the decoded rows"""
  params = torch.cat([dc.double()[:, :, None], codebook.double()[index.long()]], dim=2)
  degree = int(math.isqrt(params.shape[2])) - 1
  basis = oracle_sh.rsh_cart(directions(positions.double(), cam.double(), torch.float64), degree)
  return (basis.unsqueeze(1) * params).sum(-1) + 0.5


def directions(positions, cam, dtype):
  """unit view directions as the kernels form them: subtract, one square root, three divisions, all in ``dtype``"""
  d = positions.to(dtype) - cam.to(dtype).unsqueeze(0)
  return d / torch.sqrt((d * d).sum(-1, keepdim=True))


def basis_error(positions, cam, degree):
  """max |Y_float32 - Y_float64| over the directions of a case (CPU): the only float32 error of the codebook gradient"""
  y32 = oracle_sh.rsh_cart(directions(positions, cam, torch.float32), degree)
  y64 = oracle_sh.rsh_cart(directions(positions.double(), cam.double(), torch.float64), degree)
  return float((y32.double() - y64).abs().max())


def reference(dc, index, codebook, positions, cam, g_out):
  """dict(out, pre, g_dc, g_codebook, s): float64 colours, their unclamped values, the gradients of ``(out * g_out).sum()``
  and ``s[j, c] = sum over index[i] == j of |g_c(i)|`` with g the gradient that passes the clamp."""
  dc = dc.detach().double().cpu().requires_grad_(True)
  codebook = codebook.detach().double().cpu().requires_grad_(True)
  index = index.detach().cpu().long()
  positions, cam, g_out = positions.detach().double().cpu(), cam.detach().double().cpu(), g_out.detach().double().cpu()
  n, k = dc.shape[0], codebook.shape[0]
  params = torch.cat([dc[:, :, None], codebook[index]], dim=2)
  out = oracle_sh.evaluate_sh_at(params, positions, torch.arange(n), cam)
  out.backward(g_out)
  with torch.no_grad():
    pre = unclamped(dc, index, codebook, positions, cam)
    passed = ((pre > 0) & (pre < 1)).double() * g_out.abs()
    s = torch.zeros((k, 3), dtype=torch.float64).index_add_(0, index, passed)
  return dict(out=out.detach(), pre=pre, g_dc=dc.grad, g_codebook=codebook.grad, s=s)
