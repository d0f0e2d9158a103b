"""misc/kmeans.py and scene_codec.py without a GPU: the oracle's own properties (ties, the float32 emulation of the
kernel's chain inside the bound b), every ValueError path, the no-CPU-fallback error, the C entry points' argument
checks and scratch queries, and the CompressedScene container (decode, nbytes, file round trip)."""
import ctypes
import zipfile

import numpy as np
import pytest
import torch

import taichi_splatting_amd as tsa
from taichi_splatting_amd import Gaussians3D, _lib
from taichi_splatting_amd.misc import kmeans as km
from taichi_splatting_amd.scene_codec import CompressedScene, compress_scene, load_compressed
from tests import kmeans_oracle as ko


# ---- the oracle ----------------------------------------------------------------------------------------------------

def test_oracle_breaks_ties_to_the_lowest_index():
  codebook = np.array([[3., 0.], [1., 1.], [1., 1.], [0., 3.], [1., 1.]], dtype=np.float32)
  x = np.array([[1., 1.], [3., 0.], [2., 0.5], [0., 0.]], dtype=np.float32)
  index, d = ko.assign(x, codebook)
  # row 2 is at 1.25 from codes 0, 1, 2 and 4; row 3 at 2 from codes 1, 2 and 4
  assert index.tolist() == [1, 0, 0, 1] and index.dtype == np.int32
  assert d.tolist() == [0.0, 0.0, 1.25, 2.0]
  assert np.array_equal(ko.dist2_to(x, codebook, index), d)


def test_oracle_update_keeps_empty_and_weightless_codes():
  x = np.array([[1., 2.], [3., 4.], [5., 6.], [7., 8.]], dtype=np.float32)
  old = np.array([[9., 9.], [8., 8.], [7., 7.]], dtype=np.float32)
  new, counts, wsum = ko.update(x, [0, 0, 2, 2], old, weights=[1., 3., 0., 0.])
  assert counts.tolist() == [2, 0, 2] and wsum.tolist() == [4.0, 0.0, 0.0]
  assert new.tolist() == [[2.5, 3.5], [8., 8.], [7., 7.]] and new.dtype == np.float32


@pytest.mark.parametrize('d', [1, 2, 9, 24, 45, 64])
def test_float32_chain_stays_inside_the_bound(d):
  """The derivation of b, held to a float32 emulation of the kernel's chain on every one of the N K pairs (codes planted
  1e-4 from points, where the score nearly cancels against ||x||^2)."""
  rng = np.random.default_rng(d)
  x = rng.standard_normal((1000, d)).astype(np.float32)
  codebook = rng.standard_normal((70, d)).astype(np.float32)
  codebook[:35] = x[:35] + np.float32(1e-4) * rng.standard_normal((35, d)).astype(np.float32)
  err = np.abs(ko.emulate_scores(x, codebook).astype(np.float64) - ko.exact_scores(x, codebook))
  bound = ko.score_bound_matrix(x, codebook)
  assert (err <= bound).all(), float((err / bound).max())
  assert float((err / bound).max()) < 0.5              # the factor 2 of slack is there
  index, _ = ko.assign(x, codebook)
  # the per-point form is the same number as the matrix form (float64 summation order aside)
  assert np.allclose(ko.score_bound(x, codebook, index), bound[np.arange(1000), index], rtol=1e-12, atol=0)


# ---- validation ----------------------------------------------------------------------------------------------------

def f32(*shape):
  return torch.zeros(shape, dtype=torch.float32)


def i32(*shape):
  return torch.zeros(shape, dtype=torch.int32)


@pytest.mark.parametrize('d', [0, 65])
def test_dimension_outside_1_to_64_is_refused(d):
  with pytest.raises(ValueError, match="columns"):
    km.kmeans_assign(f32(10, d), f32(4, d))
  with pytest.raises(ValueError, match="columns"):
    km.kmeans_update(f32(10, d), i32(10), f32(4, d))
  with pytest.raises(ValueError, match="columns"):
    km.kmeans(f32(10, d), 4)
  with pytest.raises(ValueError):
    km.assign_scratch_bytes(10, d, 4)
  with pytest.raises(ValueError):
    km.update_scratch_bytes(10, d, 4)


@pytest.mark.parametrize('k', [0, 65537])
def test_code_count_outside_1_to_65536_is_refused(k):
  with pytest.raises(ValueError, match="rows"):
    km.kmeans_assign(f32(10, 9), f32(k, 9))
  with pytest.raises(ValueError, match="rows"):
    km.kmeans_update(f32(10, 9), i32(10), f32(k, 9))
  with pytest.raises(ValueError, match="k must be"):
    km.kmeans(f32(70000, 2), k)
  with pytest.raises(ValueError):
    km.assign_scratch_bytes(10, 9, k)


def test_more_codes_than_points_is_refused():
  with pytest.raises(ValueError, match="at least as many points"):
    km.kmeans(f32(10, 9), 11)


def test_wrong_dtypes_and_shapes_are_refused():
  x, c = f32(10, 9), f32(4, 9)
  for bad_x in (x.double(), x.half(), f32(10), f32(10, 9, 1), "x"):
    with pytest.raises(ValueError):
      km.kmeans_assign(bad_x, c)
    with pytest.raises(ValueError):
      km.kmeans(bad_x, 4)
  for bad_c in (c.double(), f32(4, 8), f32(4), None):
    with pytest.raises(ValueError):
      km.kmeans_assign(x, bad_c)
  for bad_index in (torch.zeros(10, dtype=torch.int64), i32(9), i32(10, 1)):
    with pytest.raises(ValueError, match="index"):
      km.kmeans_update(x, bad_index, c)
  for bad_w in (torch.ones(10, dtype=torch.float64), torch.ones(9), torch.ones(10, 1)):
    with pytest.raises(ValueError, match="weights"):
      km.kmeans_update(x, i32(10), c, bad_w)
    with pytest.raises(ValueError, match="weights"):
      km.kmeans(x, 4, weights=bad_w)
  scratch = torch.zeros(1 << 20, dtype=torch.uint8)
  with pytest.raises(ValueError, match="out_index"):
    km.kmeans_assign_into(x, c, torch.zeros(10, dtype=torch.int64), None, scratch)
  with pytest.raises(ValueError, match="out_dist2"):
    km.kmeans_assign_into(x, c, i32(10), f32(9), scratch)
  with pytest.raises(ValueError, match="out_counts"):
    km.kmeans_update_into(x, i32(10), c, i32(5), scratch)
  for bad_k, bad_it in ((4.0, 1), (True, 1), (4, -1), (4, 1.5)):
    with pytest.raises(ValueError):
      km.kmeans(x, bad_k, iterations=bad_it)


def test_negative_or_non_finite_values_are_refused():
  x = torch.randn(10, 9)
  w = torch.ones(10)
  w[3] = -1.0
  with pytest.raises(ValueError, match="non-negative"):
    km.kmeans(x, 4, weights=w)
  w[3] = float('nan')
  with pytest.raises(ValueError, match="non-negative"):
    km.kmeans(x, 4, weights=w)
  x[2, 2] = float('inf')
  with pytest.raises(ValueError, match="finite"):
    km.kmeans(x, 4)


def test_there_is_no_cpu_fallback():
  x, c = torch.randn(10, 9), torch.randn(4, 9)
  scratch = torch.zeros(1 << 20, dtype=torch.uint8)
  calls = (lambda: km.kmeans_assign(x, c), lambda: km.kmeans_update(x, i32(10), c), lambda: km.kmeans(x, 4),
           lambda: km.kmeans_assign_into(x, c, i32(10), f32(10), scratch),
           lambda: km.kmeans_update_into(x, i32(10), c, i32(4), scratch),
           lambda: compress_scene(scene(20, 3), sh_codes=4))
  for call in calls:
    with pytest.raises(RuntimeError, match="no CPU fallback"):
      call()


def test_c_entry_points_check_their_arguments(lib):
  n = ctypes.c_size_t(0)
  for d, k, word in ((0, 4, b'd must'), (65, 4, b'd must'), (9, 0, b'k must'), (9, 65537, b'k must')):
    assert lib.ms_kmeans_assign(None, 10, d, None, k, None, None, None, ctypes.byref(n), None) == -1
    assert word in lib.ms_last_error_string()
    assert lib.ms_kmeans_update(None, None, None, 10, d, k, None, None, None, None, ctypes.byref(n), None) == -1
    assert word in lib.ms_last_error_string()
  assert lib.ms_kmeans_assign(None, -1, 9, None, 4, None, None, None, ctypes.byref(n), None) == -1
  assert lib.ms_kmeans_assign(None, 1 << 31, 9, None, 4, None, None, None, ctypes.byref(n), None) == -1
  assert lib.ms_kmeans_assign(None, 10, 9, None, 4, None, None, None, None, None) == -1
  assert b'tmp_bytes' in lib.ms_last_error_string()
  # a scratch that is too small and null pointers are caught before any launch (the pointers are never followed)
  short = ctypes.c_size_t(16)
  assert lib.ms_kmeans_assign(None, 10, 9, None, 4, None, None, 1, ctypes.byref(short), None) == -3
  assert lib.ms_kmeans_update(None, None, None, 10, 9, 4, None, None, None, 1, ctypes.byref(short), None) == -3
  big = ctypes.c_size_t(1 << 30)
  assert lib.ms_kmeans_assign(None, 10, 9, None, 4, None, None, 1, ctypes.byref(big), None) == -1
  assert b'x is null' in lib.ms_last_error_string()
  assert lib.ms_kmeans_update(None, None, None, 10, 9, 4, None, None, None, 1, ctypes.byref(big), None) == -1
  assert b'codebook is null' in lib.ms_last_error_string()


def test_scratch_queries_are_host_arithmetic():
  pad = lambda v, a: (v + a - 1) // a * a
  for n, d, k in ((0, 1, 1), (1000, 9, 70), (300, 45, 4100), (64, 64, 65536)):
    kp, dp = pad(k, _lib.KMEANS_CHUNK), pad(d, 8)
    assert km.assign_scratch_bytes(n, d, k) == pad(kp * dp * 4, 256) + pad(kp * 4, 256)
    chunks = (n + _lib.KMEANS_UPDATE_CHUNK - 1) // _lib.KMEANS_UPDATE_CHUNK + k
    least = 4 * pad(4 * n, 256) + 2 * pad(4 * (k + 1), 256) + pad(chunks * (d + 1) * 8, 256)
    assert km.update_scratch_bytes(n, d, k) >= least
  assert km.MAX_D == 64 and km.MAX_K == 65536


def test_binding_constants_are_the_header_s():
  import re
  from pathlib import Path
  text = (Path(__file__).resolve().parent.parent / 'include' / 'mi355_splat.h').read_text()
  macro = lambda name: int(re.search(rf'#define {name} (\d+)', text).group(1))
  assert macro('MS_KMEANS_MAX_D') == _lib.KMEANS_MAX_D and macro('MS_KMEANS_MAX_K') == _lib.KMEANS_MAX_K
  assert macro('MS_KMEANS_CHUNK') == _lib.KMEANS_CHUNK and macro('MS_KMEANS_UPDATE_CHUNK') == _lib.KMEANS_UPDATE_CHUNK


# ---- the container -------------------------------------------------------------------------------------------------

def scene(n, degree, seed=0):
  g = torch.Generator().manual_seed(seed)
  r = lambda *shape: torch.randn(*shape, generator=g)
  return Gaussians3D(position=r(n, 3), log_scaling=r(n, 3), rotation=r(n, 4), alpha_logit=r(n, 1),
                     feature=r(n, 3, (degree + 1) ** 2), batch_size=(n,))


def compressed(n=50, k=7, degree=3, seed=0):
  s = scene(n, degree, seed)
  g = torch.Generator().manual_seed(seed + 1)
  m = (degree + 1) ** 2 - 1
  return CompressedScene(position=s.position, log_scaling=s.log_scaling, rotation=s.rotation, alpha_logit=s.alpha_logit,
                         dc=s.feature[:, :, 0].clone(), sh_codebook=torch.randn(k, 3, m, generator=g),
                         sh_index=torch.randint(0, k, (n,), generator=g, dtype=torch.int32), sh_degree=degree)


@pytest.mark.parametrize('degree', [1, 2, 3])
def test_decode_is_dc_beside_the_indexed_codes(degree):
  c = compressed(degree=degree)
  g = c.decode()
  assert isinstance(g, Gaussians3D) and g.feature.shape == (50, 3, (degree + 1) ** 2)
  assert torch.equal(g.feature, torch.cat([c.dc.unsqueeze(2), c.sh_codebook[c.sh_index.long()]], dim=2))
  for name in ('position', 'log_scaling', 'rotation', 'alpha_logit'):
    assert torch.equal(getattr(g, name), getattr(c, name))
  assert torch.equal(c.decode(device='cpu').feature, g.feature)


def test_nbytes_counts_the_stored_form():
  c = compressed(n=50, k=7, degree=3)
  assert c.nbytes == 50 * (4 * (3 + 3 + 4 + 1 + 3) + 2) + 7 * 45 * 4
  assert 50 * 58 == 50 * (4 * 14 + 2)                      # the 58 bytes per degree-3 row of the module docstring
  assert compressed(n=10, k=3, degree=1).nbytes == 10 * 58 + 3 * 9 * 4


def test_file_round_trip_is_bit_exact_and_holds_no_pickle(tmp_path):
  c = compressed(n=300, k=290, degree=2)
  c.sh_index[0] = 289
  path = tmp_path / 'scene.npz'
  c.save(path)
  with zipfile.ZipFile(path) as z:
    assert all(info.compress_type == zipfile.ZIP_STORED for info in z.infolist())      # uncompressed
  with np.load(path, allow_pickle=False) as data:                                      # would raise on an object array
    assert data['sh_index'].dtype == np.uint16 and data['sh_index'].shape == (300,)
    assert all(data[name].dtype != object for name in data.files)
  back = load_compressed(path)
  assert back.sh_degree == 2 and back.sh_index.dtype == torch.int32
  for name in ('position', 'log_scaling', 'rotation', 'alpha_logit', 'dc', 'sh_codebook', 'sh_index'):
    assert torch.equal(getattr(back, name), getattr(c, name)), name
  assert torch.equal(back.decode().feature, c.decode().feature) and back.nbytes == c.nbytes
  c.save(tmp_path / 'bare')                                 # np.savez appends .npz
  assert (tmp_path / 'bare.npz').exists()
  assert torch.equal(load_compressed(tmp_path / 'bare').sh_index, c.sh_index)
  np.savez(tmp_path / 'other.npz', position=np.zeros((3, 3), dtype=np.float32))
  with pytest.raises(ValueError, match="not a compressed scene"):
    load_compressed(tmp_path / 'other.npz')


def test_an_index_of_65535_survives_the_file(tmp_path):
  c = compressed(n=4, k=3, degree=1)
  big = CompressedScene(position=c.position, log_scaling=c.log_scaling, rotation=c.rotation, alpha_logit=c.alpha_logit,
                        dc=c.dc, sh_codebook=torch.zeros(65536, 3, 3), sh_index=torch.tensor([0, 65535, 32768, 1], dtype=torch.int32),
                        sh_degree=1)
  big.save(tmp_path / 'big.npz')
  assert load_compressed(tmp_path / 'big.npz').sh_index.tolist() == [0, 65535, 32768, 1]


def test_scenes_with_nothing_to_quantise_are_refused():
  s = scene(20, 0)
  with pytest.raises(ValueError, match="nothing to quantise"):
    compress_scene(s)
  with pytest.raises(ValueError, match="nothing to quantise"):
    compress_scene(s.replace(feature=torch.rand(20, 3)))
  with pytest.raises(ValueError, match="nothing to quantise"):
    s.compressed()
  s3 = scene(20, 3)
  with pytest.raises(ValueError, match="at least as many"):
    compress_scene(s3, sh_codes=21)
  for bad in (0, 65537, 4.0):
    with pytest.raises(ValueError, match="sh_codes"):
      compress_scene(s3, sh_codes=bad)
  with pytest.raises(ValueError, match="non-negative"):
    compress_scene(s3, sh_codes=4, weights=-torch.ones(20))
  with pytest.raises(ValueError, match="float32"):
    compress_scene(s3.replace(position=s3.position.double()), sh_codes=4)
  with pytest.raises(ValueError):
    CompressedScene(position=s3.position, log_scaling=s3.log_scaling, rotation=s3.rotation, alpha_logit=s3.alpha_logit,
                    dc=s3.feature[:, :, 0], sh_codebook=torch.zeros(4, 3, 8), sh_index=i32(20), sh_degree=3)


def test_tools_list_their_options_and_refuse_to_run_without_a_gpu():
  import subprocess
  import sys
  tools = _lib.PACKAGE_DIR.parent / 'tools'
  done = subprocess.run([sys.executable, str(tools / 'render_scene.py'), '--help'], capture_output=True, text=True, timeout=120)
  assert done.returncode == 0 and '--sh-codes' in done.stdout, done.stderr[-500:]
  done = subprocess.run([sys.executable, str(tools / 'bench_kmeans.py'), '--help'], capture_output=True, text=True, timeout=120)
  assert done.returncode == 0 and '--chunk' in done.stdout and 'cdist' in done.stdout, done.stderr[-500:]
  if not torch.cuda.is_available():
    done = subprocess.run([sys.executable, str(tools / 'bench_kmeans.py'), '--n', '1000'], capture_output=True, text=True, timeout=120)
    assert done.returncode != 0 and 'no GPU visible' in done.stderr


def test_names_are_public_and_installed():
  for name in ('kmeans', 'kmeans_assign', 'kmeans_update', 'KMeansResult', 'compress_scene', 'load_compressed', 'CompressedScene'):
    assert name in tsa.__all__ and hasattr(tsa, name)
  assert tsa.compress_scene is compress_scene and tsa.kmeans is km.kmeans
  tsa.install_as_taichi_splatting()
  import importlib
  assert importlib.import_module('taichi_splatting.misc.kmeans') is km
  assert importlib.import_module('taichi_splatting.scene_codec').CompressedScene is CompressedScene
  assert tsa.__version__ == '0.5.1'
