"""taichi_splatting_amd — MI355X (gfx950) native back end for the taichi_splatting render path.

Same public surface as the reference package (``taichi_splatting/__init__.py:1-33``); every
device stage is a hand-written HIP kernel in ``csrc/`` reached through the C-ABI of
``include/mi355_splat.h``.  ``install_as_taichi_splatting()`` registers this package under the
reference's import name so existing callers run unchanged.
"""
from .renderer import render_gaussians, render_projected, viewspace_gradient
from .rendering import Rendering, RenderedPoints
from .data_types import Gaussians2D, Gaussians3D, RasterConfig
from .mapper.tile_mapper import map_to_tiles, pad_to_tile
from .rasterizer import rasterize, rasterize_with_tiles, RasterOut
from .rasterizer.wide import rasterize_wide, render_features
from .spherical_harmonics import evaluate_sh_at, sh_rotation_matrices, rotate_sh
from . import perspective
from . import cuda_lib
from . import cuda_lib as hip_lib
from . import optim
from .perspective import CameraParams
from .taichi_queue import TaichiQueue, taichi_queue, queued
from .loss import l1_ssim_loss, ssim
from .scene_io import load_ply, save_ply, read_ply_header, load_points_ply
from .misc.coverage import camera_coverage, pack_cameras, Coverage
from .misc.relocate import relocate_gaussians3d, perturb_positions
from .optim.relocate import relocate, RelocateResult
from .misc.kmeans import kmeans, kmeans_assign, kmeans_update, KMeansResult
from .scene_codec import compress_scene, load_compressed, CompressedScene, render_compressed
from .spherical_harmonics import evaluate_sh_coded, make_coded_sh_plan, CodedSHPlan
from .appearance import apply_bilateral_grid, BilateralGrids, identity_bilateral_grid, bilateral_grid_tv
from .geometry import gaussian_normals, render_geometry, GeometryImages, normal_consistency_loss, normal_consistency
from .fusion import TSDFVolume, TriangleMesh, save_mesh_ply, fuse_scene
from .mesh import (MeshComponents, mesh_components, select_faces, remove_small_components, vertex_normals,
                   vertex_normal_sums, with_vertex_normals, simplify_mesh)
from .misc.knn import knn_query
from .mesh_eval import (SurfaceSamples, SurfaceMetrics, face_area_cdf, sample_mesh_points, surface_distances,
                        surface_metrics, metrics_from_distances, evaluate_mesh)

__version__ = '0.5.1'       # = MS_VERSION 501 of include/mi355_splat.h (tests/test_abi.py holds the two together)

__all__ = [
  'render_gaussians', 'Rendering',
  'map_to_tiles', 'pad_to_tile',
  'Gaussians2D', 'Gaussians3D',
  'RasterConfig', 'evaluate_sh_at', 'sh_rotation_matrices', 'rotate_sh',
  'rasterize', 'rasterize_with_tiles', 'rasterize_wide', 'render_features',
  'perspective', 'TaichiQueue',
  'l1_ssim_loss', 'ssim',
  'load_ply', 'save_ply', 'read_ply_header',
  'camera_coverage', 'pack_cameras', 'Coverage',
  'relocate', 'RelocateResult', 'relocate_gaussians3d', 'perturb_positions',
  'kmeans', 'kmeans_assign', 'kmeans_update', 'KMeansResult',
  'compress_scene', 'load_compressed', 'CompressedScene',
  'render_compressed', 'evaluate_sh_coded', 'make_coded_sh_plan', 'CodedSHPlan',
  'apply_bilateral_grid', 'BilateralGrids', 'identity_bilateral_grid', 'bilateral_grid_tv',
  'gaussian_normals', 'render_geometry', 'GeometryImages', 'normal_consistency_loss', 'normal_consistency',
  'TSDFVolume', 'TriangleMesh', 'save_mesh_ply', 'fuse_scene',
  'MeshComponents', 'mesh_components', 'select_faces', 'remove_small_components', 'vertex_normals', 'vertex_normal_sums',
  'with_vertex_normals', 'simplify_mesh',
  'knn_query', 'SurfaceSamples', 'SurfaceMetrics', 'face_area_cdf', 'sample_mesh_points', 'surface_distances',
  'surface_metrics', 'metrics_from_distances', 'evaluate_mesh', 'load_points_ply',
]


def install_as_taichi_splatting():
  """Register this package (and its submodules) as ``taichi_splatting`` in ``sys.modules``."""
  import importlib
  import sys
  me = sys.modules[__name__]
  sys.modules.setdefault('taichi_splatting', me)
  for sub in ('data_types', 'scene_io', 'renderer', 'rendering', 'taichi_queue', 'spherical_harmonics',
              'perspective', 'perspective.params',
              'perspective.projection', 'mapper', 'mapper.tile_mapper', 'rasterizer',
              'rasterizer.function', 'rasterizer.wide', 'cuda_lib', 'misc', 'misc.renderer2d', 'misc.morton_sort', 'misc.knn', 'misc.coverage', 'misc.relocate', 'misc.kmeans', 'scene_codec', 'appearance', 'geometry', 'fusion', 'mesh', 'mesh_eval', 'optim', 'optim.fractional', 'optim.relocate',
              'optim.visibility_aware', 'optim.parameter_class', 'optim.util', 'benchmarks', 'benchmarks.util',
              'benchmarks.bench_projection', 'benchmarks.bench_rasterizer', 'benchmarks.bench_tilemapper',
              'benchmarks.bench_sh', 'examples',
              'examples.fit_image_gaussians', 'examples.finetune_compressed', 'examples.fit_appearance'):
    mod = importlib.import_module(f'{__name__}.{sub}')
    sys.modules.setdefault(f'taichi_splatting.{sub}', mod)
  # module names of the reference whose contents live elsewhere here: evaluate_sh_at (reference
  # indexed_spherical_harmonics.py:166) is in spherical_harmonics, restore_grad (optim/autograd.py) in optim.fractional
  for alias, target in (('indexed_spherical_harmonics', 'spherical_harmonics'), ('optim.autograd', 'optim.fractional')):
    sys.modules.setdefault(f'taichi_splatting.{alias}', importlib.import_module(f'{__name__}.{target}'))
  # the reference keeps its scene generators under tests/ (tests/random_data.py)
  testing = importlib.import_module(f'{__name__}.testing')
  sys.modules.setdefault('taichi_splatting.tests', testing)
  sys.modules.setdefault('taichi_splatting.tests.random_data', importlib.import_module(f'{__name__}.testing.random_data'))
  return me
