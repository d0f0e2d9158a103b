"""The byte counts of every ``(tmp, tmp_bytes)`` entry point and every field of ``ms_frame_layout``, pinned as literals.

The numbers were recorded from the library as it stood before the scratch layouts moved to the one carver of
``csrc/common.h`` (they are part of the C-ABI's behaviour: callers cache them and carve their own blocks by them).  Every
sized dimension is taken through 0 and 1 where the entry point admits them (image and grid sides start at 1), through
one value just below and one just above a 256-byte boundary of the array it sizes, and through a mid-sized case.  The same
table drives the protocol checks: a null ``tmp_bytes`` is MS_ERR_BAD_ARG, a short block MS_ERR_TMP_TOO_SMALL (MS_ERR_BAD_ARG
for ``ms_knn_points``, as its header comment documents) with the one message text.  No call here reaches a launch: the
argument checks come first, so no GPU is needed."""
import ctypes

import pytest

from taichi_splatting_amd import _lib
from taichi_splatting_amd.rasterizer import RasterConfig

F32, F64 = _lib.MS_F32, _lib.MS_F64
FAKE = 256   # a non-null, 256-byte aligned `tmp` that is never followed
COUNTS = (0, 1, 63, 64, 65, 1000, 131072, 131073, 1000000)


@pytest.fixture(scope='module')
def lib():
  return _lib.load()


# name -> (call(lib, args, tmp, size_ref), [args, ...]); data pointers are null throughout
CASES = {
  'ms_exclusive_scan_i32': (
    lambda lib, a, tmp, ref: lib.ms_exclusive_scan_i32(None, a[0], None, None, tmp, ref, None),
    [(n,) for n in COUNTS]),
  'ms_radix_sort_pairs': (
    lambda lib, a, tmp, ref: lib.ms_radix_sort_pairs(None, None, None, None, a[0], a[1], 0, a[1] * 8, tmp, ref, None),
    [(n, kb) for kb in (4, 8) for n in COUNTS]),
  'ms_depth_argsort': (
    lambda lib, a, tmp, ref: lib.ms_depth_argsort(None, a[0], a[1], 0.0, 1.0, a[2], None, None, tmp, ref, None),
    [(n, 0, F32) for n in COUNTS] + [(1000, 1, F64)]),
  'ms_map_tiles_direct': (
    lambda lib, a, tmp, ref: lib.ms_map_tiles_direct(None, None, F32, None, a[0], a[2], a[3], 16, 0.01, 0, 1 << 30, 0, 0.0, 1.0,
                                                     a[1], None, None, None, tmp, ref, None),
    [(1000, k, 256, 128) for k in (0, 1, 31, 32, 33, 63, 64, 65, 5000, 1000000)] + [(0, 5000, 4096, 4096)]),
  'ms_knn_points': (
    lambda lib, a, tmp, ref: lib.ms_knn_points(None, None, a[0], a[1], None, None, None, tmp, ref, None),
    [(n, 3) for n in (0, 1, 15, 16, 17, 255, 256, 257, 4096, 4097, 100000)] + [(1000, 1), (1000, 8)]),
  'ms_densify_plan': (
    lambda lib, a, tmp, ref: lib.ms_densify_plan(None, None, a[0], a[1], None, None, None, tmp, ref, None),
    [(n, 2) for n in COUNTS] + [(1000, 1), (65536, 4), (65537, 4)]),
  'ms_photometric_fwd': (
    lambda lib, a, tmp, ref: lib.ms_photometric_fwd(None, None, a[0], a[1], a[2], a[3], a[4], 0.2, None, None, None, tmp, ref,
                                                    None, None),
    [(h, w, c, dt, pad) for dt in (F32, F64) for (h, w, c, pad) in (
      (1, 1, 1, _lib.PAD_SAME), (16, 16, 3, _lib.PAD_SAME), (17, 16, 3, _lib.PAD_SAME), (64, 64, 3, _lib.PAD_SAME),
      (64, 64, 3, _lib.PAD_VALID), (250, 130, 3, _lib.PAD_SAME), (255, 257, 1, _lib.PAD_SAME), (1080, 1920, 3, _lib.PAD_VALID))]),
  'ms_bilagrid_bwd': (
    lambda lib, a, tmp, ref: lib.ms_bilagrid_bwd(None, None, None, a[0], a[1], a[2], a[3], a[4], a[5], None, None, tmp, ref, None),
    [(h, w, l, gy, gx, dt) for dt in (F32, F64) for (h, w, l, gy, gx) in (
      (1, 1, 1, 1, 1), (64, 64, 8, 16, 16), (250, 130, 8, 16, 16), (1080, 1920, 8, 16, 16), (1080, 1920, 4, 8, 12),
      (37, 53, 3, 5, 7))]),
  'ms_normal_consistency_fwd': (
    lambda lib, a, tmp, ref: lib.ms_normal_consistency_fwd(None, None, None, a[0], a[1], a[2], 0, 1, 2, a[3], 0.5, tmp, ref,
                                                           None, None, None),
    [(h, w, f, dt) for dt in (F32, F64) for (h, w, f) in (
      (1, 1, 5), (100, 200, 5), (128, 128, 8), (129, 127, 8), (250, 130, 5), (1080, 1920, 8))]),
  'ms_kmeans_assign': (
    lambda lib, a, tmp, ref: lib.ms_kmeans_assign(None, a[0], a[1], None, a[2], None, None, tmp, ref, None),
    [(n, d, k) for n in (0, 1000) for (d, k) in (
      (1, 1), (8, 1), (9, 4), (45, 64), (45, 65), (64, 127), (64, 128), (64, 129), (45, 4096), (24, 65536))]),
  'ms_kmeans_update': (
    lambda lib, a, tmp, ref: lib.ms_kmeans_update(None, None, None, a[0], a[1], a[2], None, None, None, tmp, ref, None),
    [(n, 45, 256) for n in COUNTS] + [(1000, d, k) for (d, k) in ((1, 1), (9, 4), (64, 62), (64, 63), (64, 64), (45, 65536))]),
  'ms_sh_coded_bwd': (
    lambda lib, a, tmp, ref: lib.ms_sh_coded_bwd(None, None, None, None, None, None, None, a[1], a[0], a[2], a[3], None, None,
                                                 tmp, ref, None),
    [(n, min(n, chunks), 256, deg) for deg in (1, 2, 3) for (n, chunks) in (
      (0, 0), (1, 0), (1, 1), (15, 1), (16, 2), (17, 3), (1000, 5), (100000, 451), (1000000, 65536))]),
  'ms_mesh_components': (
    lambda lib, a, tmp, ref: lib.ms_mesh_components(None, a[0], a[1], None, None, None, tmp, ref, None),
    [(v, 2 * v) for v in COUNTS] + [(1000, 0), (0, 1000)]),
  'ms_mesh_component_filter': (
    lambda lib, a, tmp, ref: lib.ms_mesh_component_filter(None, a[0], 1, 0, None, a[1], None, tmp, ref, None),
    [(k, 2000) for k in COUNTS] + [(100, 0)]),
  'ms_mesh_select_plan': (
    lambda lib, a, tmp, ref: lib.ms_mesh_select_plan(None, None, a[0], a[1], None, None, None, tmp, ref, None),
    [(v, 2 * v) for v in COUNTS] + [(1000, 0), (0, 1000), (131073, 5)]),
  'ms_mesh_vertex_normals': (
    lambda lib, a, tmp, ref: lib.ms_mesh_vertex_normals(None, None, a[0], a[1], None, None, tmp, ref, None),
    [(v, f) for (v, f) in ((0, 0), (1, 0), (0, 1), (1, 1), (31, 21), (32, 21), (33, 22), (63, 43), (1000, 2000),
                           (131072, 262144), (1000000, 2000000))]),
}

# the reported sizes, in the order of the argument tuples above
EXPECTED = {
  'ms_exclusive_scan_i32': [256, 256, 256, 256, 256, 256, 256, 256, 1024],
  'ms_radix_sort_pairs': [2304, 2816, 2816, 2816, 3328, 10496, 1082624, 1084160, 8252160, 2304, 2816, 3072, 3072,
    3584, 14592, 1606912, 1608448, 12252160],
  'ms_depth_argsort': [2304, 2816, 2816, 2816, 3328, 10496, 1082624, 1084160, 8252160, 10496],
  'ms_map_tiles_direct': [3328, 3328, 3328, 3328, 3840, 3840, 3840, 4864, 124160, 24252160, 124160],
  'ms_knn_points': [0, 768, 768, 768, 1024, 4608, 4608, 4864, 66048, 66816, 1612800, 16640, 16640],
  'ms_densify_plan': [256, 256, 256, 256, 256, 256, 256, 512, 2048, 256, 256, 256],
  'ms_photometric_fwd': [256, 256, 256, 256, 256, 1024, 768, 49152, 256, 256, 256, 256, 256, 1792, 1280, 98048],
  'ms_bilagrid_bwd': [256, 196608, 196608, 2949120, 1105920, 10240, 256, 196608, 196608, 2949120, 1105920, 10240],
  'ms_normal_consistency_fwd': [256, 256, 256, 256, 512, 16384, 256, 256, 256, 256, 512, 16384],
  'ms_kmeans_assign': [4608, 4608, 8704, 25088, 25088, 33280, 33280, 66560, 802816, 6553600, 4608, 4608, 8704, 25088,
    25088, 33280, 33280, 66560, 802816, 6553600],
  'ms_kmeans_update': [99072, 101120, 101120, 101120, 102656, 124160, 3323648, 3326720, 24708608, 27648, 27904,
    60160, 60672, 61952, 24669440],
  'ms_sh_coded_bwd': [256, 512, 512, 768, 768, 768, 24576, 2432512, 28718592, 256, 512, 512, 768, 1024, 1280, 25088,
    2486784, 36582912, 512, 768, 768, 1024, 1280, 1792, 26112, 2562560, 47592960],
  'ms_mesh_components': [1024, 1024, 1024, 1280, 1536, 8704, 1049344, 1049600, 8001536, 8704, 1024],
  'ms_mesh_component_filter': [3584, 4096, 4096, 4096, 5888, 30976, 3704064, 3706880, 28252160, 5888],
  'ms_mesh_select_plan': [512, 512, 512, 512, 512, 512, 512, 768, 2304, 512, 512, 512],
  'ms_mesh_vertex_normals': [3584, 3584, 4096, 4096, 4096, 4096, 5888, 7424, 155904, 20120832, 153501440],
}

FRAME_FIELDS = [name for name, _ in _lib.FrameLayoutC._fields_]
# (dtype, projected_input, sh_degree, split_long_runs, n, k_capacity) at 250 x 130, three channels, tile 16
FRAME_CASES = [(dt, proj, deg, split, n, k)
               for dt in (F32, F64) for (proj, deg) in ((0, -1), (0, 3), (1, -1)) for split in (0, 1)
               for (n, k) in ((0, 0), (1, 1), (63, 64), (65, 63), (1000, 5000))]
# every field of ms_frame_layout (FRAME_FIELDS order) for each of FRAME_CASES
FRAME_EXPECTED = [
  (2816, 4352, 512, 3072, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (2816, 5376, 512, 3584, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (4352, 6912, 512, 4096, 0, 1792, 2048, 2816, 2304, 2560, 2816, 0, 256, 512, 768, 1024, 3072, 0, 0, 512, 768, 1280, 4096, 256),
  (4864, 9216, 512, 4096, 0, 2048, 2560, 4096, 2816, 3072, 3328, 0, 512, 1024, 1536, 2048, 4352, 0, 0, 512, 768, 1280, 4608, 256),
  (34560, 64000, 20480, 144384, 0, 28160, 32256, 44544, 32512, 32768, 33024, 0, 4096, 8192, 12288, 16384, 44800, 0, 0, 40192, 60416, 100608, 34304, 20224),
  (2816, 4352, 512, 3072, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (2816, 5376, 9216, 3584, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (4352, 6912, 9216, 4096, 0, 1792, 2048, 2816, 2304, 2560, 2816, 0, 256, 512, 768, 1024, 3072, 0, 0, 512, 768, 1280, 4096, 256),
  (4864, 9216, 9216, 4096, 0, 2048, 2560, 4096, 2816, 3072, 3328, 0, 512, 1024, 1536, 2048, 4352, 0, 0, 512, 768, 1280, 4608, 256),
  (34560, 64000, 45568, 144384, 0, 28160, 32256, 44544, 32512, 32768, 33024, 0, 4096, 8192, 12288, 16384, 44800, 0, 0, 40192, 60416, 100608, 34304, 20224),
  (2816, 4352, 512, 3072, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (2816, 5376, 512, 3584, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (4864, 6912, 512, 4096, 0, 1792, 2048, 2816, 2816, 3072, 3328, 0, 256, 512, 768, 1024, 3072, 0, 0, 512, 768, 1280, 4608, 256),
  (5632, 9216, 512, 4096, 0, 2048, 2560, 4096, 3584, 3840, 4096, 0, 512, 1024, 1536, 2048, 4352, 0, 0, 512, 768, 1280, 5376, 256),
  (46336, 64000, 20480, 144384, 0, 28160, 32256, 44544, 44288, 44544, 44800, 0, 4096, 8192, 12288, 16384, 44800, 0, 0, 40192, 60416, 100608, 46080, 20224),
  (2816, 4352, 512, 3072, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (2816, 5376, 9216, 3584, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (4864, 6912, 9216, 4096, 0, 1792, 2048, 2816, 2816, 3072, 3328, 0, 256, 512, 768, 1024, 3072, 0, 0, 512, 768, 1280, 4608, 256),
  (5632, 9216, 9216, 4096, 0, 2048, 2560, 4096, 3584, 3840, 4096, 0, 512, 1024, 1536, 2048, 4352, 0, 0, 512, 768, 1280, 5376, 256),
  (46336, 64000, 45568, 144384, 0, 28160, 32256, 44544, 44288, 44544, 44800, 0, 4096, 8192, 12288, 16384, 44800, 0, 0, 40192, 60416, 100608, 46080, 20224),
  (2816, 4352, 512, 3072, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (2816, 5376, 512, 3584, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (2816, 6912, 512, 4096, 0, 256, 512, 2816, 768, 1024, 1280, 0, 256, 512, 768, 1024, 3072, 0, 0, 512, 768, 1280, 2560, 256),
  (2816, 9216, 512, 4096, 0, 256, 512, 4096, 768, 1024, 1280, 0, 512, 1024, 1536, 2048, 4352, 0, 0, 512, 768, 1280, 2560, 256),
  (2816, 64000, 20480, 144384, 0, 256, 512, 44544, 768, 1024, 1280, 0, 4096, 8192, 12288, 16384, 44800, 0, 0, 40192, 60416, 100608, 2560, 20224),
  (2816, 4352, 512, 3072, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (2816, 5376, 9216, 3584, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (2816, 6912, 9216, 4096, 0, 256, 512, 2816, 768, 1024, 1280, 0, 256, 512, 768, 1024, 3072, 0, 0, 512, 768, 1280, 2560, 256),
  (2816, 9216, 9216, 4096, 0, 256, 512, 4096, 768, 1024, 1280, 0, 512, 1024, 1536, 2048, 4352, 0, 0, 512, 768, 1280, 2560, 256),
  (2816, 64000, 45568, 144384, 0, 256, 512, 44544, 768, 1024, 1280, 0, 4096, 8192, 12288, 16384, 44800, 0, 0, 40192, 60416, 100608, 2560, 20224),
  (2816, 4352, 512, 3072, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (2816, 5376, 512, 3584, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (6400, 8448, 512, 4096, 0, 3584, 4096, 2816, 4352, 4608, 4864, 0, 256, 512, 768, 1024, 4608, 0, 0, 512, 768, 1280, 6144, 256),
  (6912, 11008, 512, 4096, 0, 3840, 4608, 4096, 4864, 5120, 5376, 0, 512, 1024, 1536, 2048, 6144, 0, 0, 512, 768, 1280, 6656, 256),
  (66560, 91904, 20480, 144384, 0, 56064, 64256, 44544, 64512, 64768, 65024, 0, 4096, 8192, 12288, 16384, 72704, 0, 0, 40192, 60416, 100608, 66304, 20224),
  (2816, 4352, 512, 3072, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (2816, 5376, 512, 3584, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (6400, 8448, 512, 4096, 0, 3584, 4096, 2816, 4352, 4608, 4864, 0, 256, 512, 768, 1024, 4608, 0, 0, 512, 768, 1280, 6144, 256),
  (6912, 11008, 512, 4096, 0, 3840, 4608, 4096, 4864, 5120, 5376, 0, 512, 1024, 1536, 2048, 6144, 0, 0, 512, 768, 1280, 6656, 256),
  (66560, 91904, 20480, 144384, 0, 56064, 64256, 44544, 64512, 64768, 65024, 0, 4096, 8192, 12288, 16384, 72704, 0, 0, 40192, 60416, 100608, 66304, 20224),
  (2816, 4352, 512, 3072, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (2816, 5376, 512, 3584, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (7680, 8448, 512, 4096, 0, 3584, 4096, 2816, 5632, 5888, 6144, 0, 256, 512, 768, 1024, 4608, 0, 0, 512, 768, 1280, 7424, 256),
  (8448, 11008, 512, 4096, 0, 3840, 4608, 4096, 6400, 6656, 6912, 0, 512, 1024, 1536, 2048, 6144, 0, 0, 512, 768, 1280, 8192, 256),
  (90368, 91904, 20480, 144384, 0, 56064, 64256, 44544, 88320, 88576, 88832, 0, 4096, 8192, 12288, 16384, 72704, 0, 0, 40192, 60416, 100608, 90112, 20224),
  (2816, 4352, 512, 3072, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (2816, 5376, 512, 3584, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (7680, 8448, 512, 4096, 0, 3584, 4096, 2816, 5632, 5888, 6144, 0, 256, 512, 768, 1024, 4608, 0, 0, 512, 768, 1280, 7424, 256),
  (8448, 11008, 512, 4096, 0, 3840, 4608, 4096, 6400, 6656, 6912, 0, 512, 1024, 1536, 2048, 6144, 0, 0, 512, 768, 1280, 8192, 256),
  (90368, 91904, 20480, 144384, 0, 56064, 64256, 44544, 88320, 88576, 88832, 0, 4096, 8192, 12288, 16384, 72704, 0, 0, 40192, 60416, 100608, 90112, 20224),
  (2816, 4352, 512, 3072, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (2816, 5376, 512, 3584, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (2816, 8448, 512, 4096, 0, 256, 512, 2816, 768, 1024, 1280, 0, 256, 512, 768, 1024, 4608, 0, 0, 512, 768, 1280, 2560, 256),
  (2816, 11008, 512, 4096, 0, 256, 512, 4096, 768, 1024, 1280, 0, 512, 1024, 1536, 2048, 6144, 0, 0, 512, 768, 1280, 2560, 256),
  (2816, 91904, 20480, 144384, 0, 256, 512, 44544, 768, 1024, 1280, 0, 4096, 8192, 12288, 16384, 72704, 0, 0, 40192, 60416, 100608, 2560, 20224),
  (2816, 4352, 512, 3072, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (2816, 5376, 512, 3584, 0, 256, 512, 1280, 768, 1024, 1280, 0, 256, 512, 768, 1024, 1536, 0, 0, 256, 512, 768, 2560, 256),
  (2816, 8448, 512, 4096, 0, 256, 512, 2816, 768, 1024, 1280, 0, 256, 512, 768, 1024, 4608, 0, 0, 512, 768, 1280, 2560, 256),
  (2816, 11008, 512, 4096, 0, 256, 512, 4096, 768, 1024, 1280, 0, 512, 1024, 1536, 2048, 6144, 0, 0, 512, 768, 1280, 2560, 256),
  (2816, 91904, 20480, 144384, 0, 256, 512, 44544, 768, 1024, 1280, 0, 4096, 8192, 12288, 16384, 72704, 0, 0, 40192, 60416, 100608, 2560, 20224),
]


def frame_layout(lib, case):
  dt, proj, deg, split, n, k = case
  desc = _lib.FrameDescC(n=n, k_capacity=k, image_w=250, image_h=130, dtype=dt, f=3, sh_degree=deg, depth16=0,
                         tile_row_begin=0, tile_row_end=1 << 30, projected_input=proj, mapper=_lib.MAPPER_DIRECT,
                         split_long_runs=split, split_seg_len=0, sh_active_bands=0, near_plane=0.1, far_plane=100.0,
                         blur_cov=0.3, clamp_margin=0.15, raster=_lib.raster_config_c(RasterConfig()))
  lay = _lib.FrameLayoutC()
  assert lib.ms_frame_layout_query(ctypes.byref(desc), ctypes.byref(lay)) == 0, lib.ms_last_error_string()
  return tuple(int(getattr(lay, name)) for name in FRAME_FIELDS)


def query(lib, name, args):
  call, _ = CASES[name]
  need = ctypes.c_size_t(12345)
  assert call(lib, args, None, ctypes.byref(need)) == 0, (name, args, lib.ms_last_error_string())
  return int(need.value)


def test_the_table_covers_every_entry_point_with_a_scratch_block():
  with_scratch = {name for name, (_, argtypes) in _lib.SIGNATURES.items() if ctypes.POINTER(ctypes.c_size_t) in argtypes}
  assert with_scratch == set(CASES) == set(EXPECTED)
  assert all(len(EXPECTED[name]) == len(CASES[name][1]) for name in CASES)
  assert len(FRAME_EXPECTED) == len(FRAME_CASES)


@pytest.mark.parametrize('name', sorted(CASES))
def test_reported_sizes(lib, name):
  got = [query(lib, name, args) for args in CASES[name][1]]
  assert got == EXPECTED[name], [(a, g, w) for a, g, w in zip(CASES[name][1], got, EXPECTED[name]) if g != w]
  assert all(g % 256 == 0 for g in got)


def test_frame_layout_fields(lib):
  for case, want in zip(FRAME_CASES, FRAME_EXPECTED):
    got = frame_layout(lib, case)
    assert got == want, (case, [(f, g, w) for f, g, w in zip(FRAME_FIELDS, got, want) if g != w])


@pytest.mark.parametrize('name', sorted(CASES))
def test_protocol_errors(lib, name):
  call, cases = CASES[name]
  too_small = -1 if name == 'ms_knn_points' else -3       # ms_knn_points: MS_ERR_BAD_ARG, documented in the header
  checked = 0
  for args, need in zip(cases, EXPECTED[name]):
    assert call(lib, args, None, None) == -1 and b'tmp_bytes' in lib.ms_last_error_string(), (name, args)
    assert call(lib, args, FAKE, None) == -1, (name, args)
    if need == 0:
      continue                                            # nothing can be short of an empty block
    for short in {0, need - 1}:
      size = ctypes.c_size_t(short)
      assert call(lib, args, FAKE, ctypes.byref(size)) == too_small, (name, args, short)
      assert b'tmp_bytes too small' in lib.ms_last_error_string(), (name, args, short)
      assert size.value == short                          # a run never writes the size back
    checked += 1
  assert checked > 0
