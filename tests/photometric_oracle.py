"""float64 oracle of the photometric loss (csrc/loss.hip), the float32 torch composition it is measured against, and the
inputs and shapes the GPU tests use.  Imported by tests/test_photometric_host.py (which checks the oracle itself: a
literal restatement, gradcheck, known answers) and tests/test_gpu_photometric.py.

Definitions, per channel of (H, W, C) images, G the 11 x 11 window of exp(-k^2 / (2 1.5^2)) normalised to sum 1:
  mu1 = G*x  mu2 = G*y  s11 = G*x^2 - mu1^2  s22 = G*y^2 - mu2^2  s12 = G*xy - mu1 mu2
  ssim = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s11 + s22 + C2)),  C1 = 0.01^2, C2 = 0.03^2
  loss = (1 - lam) mean|x - y| + lam (1 - mean ssim)
'same' zero-pads like conv2d(padding=5); 'valid' gives the (H - 10, W - 10) map.  N1 = H W C, N2 = map elements.

``mutation`` serves the tests only (as in oracle/optim.py): each one is a plausible kernel bug, and
test_photometric_host.py shows that the float32 tolerance rejects every one of them.

The float32 tolerance (``tolerances``).  The float32 error of this loss is not relative to the result: it is set by the
cancellation in G*x^2 - mu1^2 against the C2 = 9e-4 of the denominator, so it depends on the input (random images: map
error 7e-6; a bright, nearly flat pair: 1.7e-3).  The bound is therefore evaluated per input from the float32 torch
composition (``torch_composition``: permute, five grouped conv2d, element-wise, autograd), the yardstick, never from the
kernel: for each compared quantity
    tol = 4 * max|composition_f32 - oracle_f64| + floor,
the factor 4 because the kernel sums the 121 taps in another order than conv2d and nothing else differs.  The floor
covers what no float32 implementation can avoid, the rounding of the result itself, 4 * 2^-24 * max|quantity|, and for
the gradient the term that remains when the true gradient cancels (identical images: float32 returns 5e-10 where the
truth is 0): 4 * 2^-24 * lam * max(|x|, |y|) / (N2 * C2).  The loss is (1 - lam) l1 + lam (1 - ssim), a difference against a
mean ssim near 1 that itself carries 2^-24 of rounding, so its bound is the bounds of its two terms propagated,
(1 - lam) tol_l1 + lam tol_ssim, plus the rounding of the result (a floor relative to the loss alone would be 0 for
identical images, where a float32 mean ssim of 1 - 1.5e-9 already rounds to 1).  Both constants c = 4 are the same
safety factor over one half-ulp (2^-24) of rounding; on the inputs below the composition's own deviation dominates the floor everywhere
except for identical images and the exactly representable l1 term.
"""
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2
RADIUS = 5
TAPS = 2 * RADIUS + 1
MUTATIONS = ('sigma_1_4', 'window_not_normalised', 'c2_c1_swapped', 'factor_2_dropped', 'c_term_uses_x', 'halo_clamped',
             'sign_dropped', 'n1_for_n2')


def window(dtype=torch.float64, mutation=None):
  sigma = 1.4 if mutation == 'sigma_1_4' else 1.5
  k = torch.arange(TAPS, dtype=torch.float64) - RADIUS
  g = torch.exp(-k * k / (2 * sigma * sigma))
  if mutation != 'window_not_normalised':
    g = g / g.sum()
  return g.to(dtype)


def _nchw(t):
  return t.permute(2, 0, 1).unsqueeze(0)


def _hwc(t):
  return t.squeeze(0).permute(1, 2, 0)


def _filter(t, g, pad, clamp=False):
  """(1, C, H, W) filtered by the 11 x 11 window outer(g, g) per channel, zero padding ``pad`` (replicated if clamp)"""
  c = t.shape[1]
  k = torch.outer(g, g).expand(c, 1, TAPS, TAPS).contiguous()
  if clamp and pad:
    return F.conv2d(F.pad(t, (pad,) * 4, mode='replicate'), k, groups=c)
  return F.conv2d(t, k, padding=pad, groups=c)


def moments(x, y, padding='same', mutation=None):
  """(mu1, mu2, s11, s22, s12) as (1, C, Hm, Wm)"""
  g = window(x.dtype, mutation)
  pad = RADIUS if padding == 'same' else 0
  clamp = mutation == 'halo_clamped'
  X, Y = _nchw(x), _nchw(y)
  mu1, mu2 = _filter(X, g, pad, clamp), _filter(Y, g, pad, clamp)
  s11 = _filter(X * X, g, pad, clamp) - mu1 * mu1
  s22 = _filter(Y * Y, g, pad, clamp) - mu2 * mu2
  s12 = _filter(X * Y, g, pad, clamp) - mu1 * mu2
  return mu1, mu2, s11, s22, s12


def _constants(mutation):
  return (C2, C1) if mutation == 'c2_c1_swapped' else (C1, C2)


def ssim_of_moments(mu1, mu2, s11, s22, s12, mutation=None):
  c1, c2 = _constants(mutation)
  return (2 * mu1 * mu2 + c1) * (2 * s12 + c2) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))


def ssim_map(x, y, padding='same', mutation=None):
  """(Hm, Wm, C)"""
  return _hwc(ssim_of_moments(*moments(x, y, padding, mutation), mutation=mutation))


def loss_terms(x, y, lam=0.2, padding='same', mutation=None):
  """(loss, l1, ssim) as 0-dim tensors, differentiable by autograd"""
  m = ssim_map(x, y, padding, mutation)
  l1 = (x - y).abs().mean()
  ssim = m.sum() / (x.numel() if mutation == 'n1_for_n2' else m.numel())
  return (1 - lam) * l1 + lam * (1 - ssim), l1, ssim


def analytic(x, y, padding='same', mutation=None):
  """Everything the kernels produce, by the formulas they implement and without autograd: dict of l1, ssim, the partial
  maps A, B, C (Hm, Wm, C) and the two halves of the gradient, grad_l1 = d l1 / dx and grad_ssim = d (mean ssim) / dx, so
  that  loss = (1 - lam) l1 + lam (1 - ssim),  dloss/dx = (1 - lam) grad_l1 - lam grad_ssim  for every lam."""
  x, y = x.detach(), y.detach()
  c1, c2 = _constants(mutation)
  mu1, mu2, s11, s22, s12 = moments(x, y, padding, mutation)
  a1, a2 = 2 * mu1 * mu2 + c1, 2 * s12 + c2
  b1, b2 = mu1 * mu1 + mu2 * mu2 + c1, s11 + s22 + c2
  f = a1 * a2 / (b1 * b2)
  df_dmu1 = 2 * mu2 * a2 / (b1 * b2) - 2 * mu1 * f / b1
  B = -f / b2
  Cm = 2 * a1 / (b1 * b2)
  A = df_dmu1 - 2 * mu1 * B - mu2 * Cm
  g = window(x.dtype, mutation)
  back = RADIUS if padding == 'same' else 2 * RADIUS       # adjoint of the filter: the same filter / the full correlation
  clamp = mutation == 'halo_clamped' and padding == 'same'
  ga, gb, gc = (_hwc(_filter(t, g, back, clamp)) for t in (A, B, Cm))
  n1 = x.numel()
  n2 = n1 if mutation == 'n1_for_n2' else f.numel()
  two = 1.0 if mutation == 'factor_2_dropped' else 2.0
  grad_ssim = (ga + two * x * gb + (x if mutation == 'c_term_uses_x' else y) * gc) / n2
  d = x - y
  grad_l1 = (d if mutation == 'sign_dropped' else torch.sign(d)) / n1
  return dict(l1=d.abs().mean(), ssim=f.sum() / n2, A=_hwc(A), B=_hwc(B), C=_hwc(Cm), grad_l1=grad_l1, grad_ssim=grad_ssim)


def combine(parts, lam):
  """(loss, dloss/dx) of ``analytic``'s parts at weight lam"""
  return ((1 - lam) * parts['l1'] + lam * (1 - parts['ssim']), (1 - lam) * parts['grad_l1'] - lam * parts['grad_ssim'])


def literal_ssim_map(x, y, padding='same'):
  """The definition once more, as a direct double loop over the window taps on a zero-padded copy: no conv2d."""
  h, w, _ = x.shape
  g = window(torch.float64)
  pad = RADIUS if padding == 'same' else 0
  hm, wm = h + 2 * pad - 2 * RADIUS, w + 2 * pad - 2 * RADIUS

  def filt(t):
    tp = torch.zeros((h + 2 * pad, w + 2 * pad, t.shape[2]), dtype=torch.float64)
    tp[pad:pad + h, pad:pad + w] = t
    out = torch.zeros((hm, wm, t.shape[2]), dtype=torch.float64)
    for dy in range(TAPS):
      for dx in range(TAPS):
        out += g[dy] * g[dx] * tp[dy:dy + hm, dx:dx + wm]
    return out

  mu1, mu2 = filt(x), filt(y)
  s11, s22, s12 = filt(x * x) - mu1 * mu1, filt(y * y) - mu2 * mu2, filt(x * y) - mu1 * mu2
  return (2 * mu1 * mu2 + C1) * (2 * s12 + C2) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))


def torch_composition(x, y, padding='same'):
  """The float32 chain a user writes in torch today (permute to NCHW, five grouped conv2d, element-wise, autograd),
  evaluated at the inputs rounded to float32: dict like ``analytic`` without the partial maps."""
  x32 = x.detach().to(torch.float32).requires_grad_(True)
  y32 = y.detach().to(torch.float32)
  m = ssim_map(x32, y32, padding)
  l1, ssim = (x32 - y32).abs().mean(), m.mean()
  grad_l1, = torch.autograd.grad(l1, x32, retain_graph=True)
  grad_ssim, = torch.autograd.grad(ssim, x32)
  return dict(l1=l1.detach(), ssim=ssim.detach(), grad_l1=grad_l1, grad_ssim=grad_ssim)


EPS = 2.0 ** -24
SAFETY = 4.0


def tolerances(x, y, lam, padding, parts=None):
  """The float32 error model of the module docstring on input (x, y): dict(loss, l1, ssim, grad) of absolute bounds.
  x, y float64 with float32-representable values; parts = analytic(x, y, padding) if already known."""
  parts = parts or analytic(x, y, padding)
  comp = torch_composition(x, y, padding)
  loss64, grad64 = combine(parts, lam)
  loss32, grad32 = combine({k: v.double() for k, v in comp.items()}, lam)
  n2 = parts['A'].numel()
  peak = float(torch.maximum(x.abs().max(), y.abs().max()))
  tol_l1 = SAFETY * float((comp['l1'].double() - parts['l1']).abs()) + SAFETY * EPS * float(parts['l1'])
  tol_ssim = SAFETY * float((comp['ssim'].double() - parts['ssim']).abs()) + SAFETY * EPS * abs(float(parts['ssim']))
  return dict(
    loss=(1 - lam) * tol_l1 + lam * tol_ssim + SAFETY * EPS * abs(float(loss64)),
    l1=tol_l1, ssim=tol_ssim,
    grad=SAFETY * float((grad32 - grad64).abs().max()) + SAFETY * EPS * float(grad64.abs().max())
         + SAFETY * EPS * lam * peak / (n2 * C2))


def _f32(t):
  return t.to(torch.float32).to(torch.float64)


def make_pair(kind, h, w, c, seed=0):
  """float64 (x, y) with float32-representable values"""
  gen = torch.Generator().manual_seed(1000 * seed + 7 * h + 3 * w + c)
  if kind == 'random':
    x, y = torch.rand((h, w, c), generator=gen, dtype=torch.float64), torch.rand((h, w, c), generator=gen, dtype=torch.float64)
  elif kind == 'smooth_noisy':
    i, j = torch.meshgrid(torch.linspace(0, 1, h, dtype=torch.float64), torch.linspace(0, 1, w, dtype=torch.float64), indexing='ij')
    y = torch.stack([0.5 + 0.4 * torch.sin(3 * i + 5 * j + k) for k in range(c)], dim=-1)
    x = (y + 0.05 * torch.randn((h, w, c), generator=gen, dtype=torch.float64)).clamp(0, 1)
  elif kind == 'bright_flat':
    y = 0.97 + 0.002 * torch.rand((h, w, c), generator=gen, dtype=torch.float64)
    x = y + 0.001 * torch.randn((h, w, c), generator=gen, dtype=torch.float64)
  elif kind == 'identical':
    x = torch.rand((h, w, c), generator=gen, dtype=torch.float64)
    y = x.clone()
  else:
    raise ValueError(kind)
  return _f32(x), _f32(y)


# (H, W, C) of the GPU tests.  The float kernels cut tiles of 32 rows x 64 floats of a W*C row, the double kernels of
# 16 rows x 64 floats: one tile exactly and one tile +- 1 in each direction for both, strips narrower than the halo.
SHAPES = (
  (1, 1, 1), (1, 1, 3), (7, 5, 3), (11, 11, 1), (11, 11, 3), (11, 11, 4), (37, 53, 3), (129, 257, 3), (129, 257, 1),
  (32, 64, 1), (31, 63, 1), (33, 65, 1), (16, 16, 4), (15, 17, 4), (17, 15, 4), (32, 16, 4), (33, 21, 3), (31, 22, 3),
  (16, 64, 1), (10, 64, 3), (64, 10, 3), (10, 10, 4), (40, 10, 1), (10, 40, 1),
)
KINDS = ('random', 'smooth_noisy', 'bright_flat', 'identical')
KIND_SHAPE = (61, 83, 3)          # the four named inputs of the float32 tests
LAMBDAS = (0.0, 0.2, 1.0)


def paddings(h, w):
  return ('same', 'valid') if min(h, w) >= TAPS else ('same',)
