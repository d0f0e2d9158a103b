"""-m gpu: scan / radix sort / ranges against torch (bit-exact integer work)."""
import numpy as np
import pytest
import torch

from taichi_splatting_amd import cuda_lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('n', [0, 1, 63, 64, 4096, 4097, 100003, 3_000_000])
def test_full_cumsum(n):
  torch.manual_seed(n)
  x = torch.randint(0, 9, (n,), dtype=torch.int32, device=DEV)
  out, total = cuda_lib.full_cumsum(x)
  want = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(x.long(), 0)])
  assert out.shape[0] == n + 1
  assert torch.equal(out.long(), want)
  assert total == int(want[-1])


@pytest.mark.parametrize('n', [1, 100, 4096, 4097, 250_001, 2_000_003])
@pytest.mark.parametrize('dtype,end_bit', [(torch.int64, 48), (torch.int64, 49), (torch.int64, 64),
                                           (torch.int32, 32), (torch.int32, 20)])
def test_radix_sort_pairs_stable(n, dtype, end_bit):
  torch.manual_seed(n + end_bit)
  bits = end_bit if end_bit < 63 else 62
  # few distinct keys in the low range => many ties => stability is exercised
  keys = torch.randint(0, 1 << min(bits, 40), (n,), dtype=torch.int64, device=DEV)
  keys[::3] = keys[::3] % 17
  if dtype == torch.int32:
    keys = (keys % (1 << min(bits, 31))).to(torch.int32)
  values = torch.arange(n, dtype=torch.int32, device=DEV)
  ko, vo = cuda_lib.radix_sort_pairs(keys, values, end_bit=end_bit)
  wk, order = torch.sort(keys.long(), stable=True)
  assert torch.equal(ko.long(), wk)
  assert torch.equal(vo.long(), order)
  # inputs untouched
  assert torch.equal(values, torch.arange(n, dtype=torch.int32, device=DEV))


def test_radix_sort_signed_and_partial_bits():
  torch.manual_seed(0)
  keys = torch.randint(-1000, 1000, (50000,), dtype=torch.int32, device=DEV)
  vals = torch.arange(50000, dtype=torch.int32, device=DEV)
  ko, vo = cuda_lib.radix_sort_pairs(keys, vals)
  wk, order = torch.sort(keys, stable=True)
  assert torch.equal(ko, wk) and torch.equal(vo.long(), order)
  # bit range [8, 16): sort by that byte only, stable
  k2 = torch.randint(0, 1 << 24, (50000,), dtype=torch.int32, device=DEV)
  ko, vo = cuda_lib.radix_sort_pairs(k2, vals, start_bit=8, end_bit=16)
  wk, order = torch.sort((k2 >> 8) & 0xff, stable=True)
  assert torch.equal((ko >> 8) & 0xff, wk) and torch.equal(vo.long(), order)
  assert torch.equal(cuda_lib.radix_argsort(keys).long(), torch.sort(keys, stable=True)[1])


def test_segmented_sort_pairs():
  torch.manual_seed(1)
  k = torch.randint(0, 100, (2000,), dtype=torch.int32, device=DEV)
  v = torch.arange(2000, dtype=torch.int32, device=DEV)
  starts = torch.tensor([0, 700, 700, 1500], dtype=torch.int64, device=DEV)
  ends = torch.tensor([700, 700, 1500, 2000], dtype=torch.int64, device=DEV)
  ko, vo = cuda_lib.segmented_sort_pairs(k, v, starts, ends)
  for s, e in zip(starts.tolist(), ends.tolist()):
    wk, order = torch.sort(k[s:e], stable=True)
    assert torch.equal(ko[s:e], wk)
    assert torch.equal(vo[s:e].long(), order + s)


@pytest.mark.parametrize('n,resolution', [(1, 0.01), (1000, 0.001), (300000, 0.01), (50000, 2.0)])
def test_morton_codes_and_argsort_match_oracle(n, resolution):
  # ms_morton_codes64 + 64-bit radix argsort against oracle/morton.py (bit-exact codes, identical stable order)
  from oracle import morton as omorton
  from taichi_splatting_amd.misc import morton_sort
  torch.manual_seed(n)
  pts = (torch.rand(n, 3) * torch.tensor([8.0, 3.0, 20.0]) - 2.0)
  if n > 10:
    pts[3] = pts[7]                                   # duplicates: stable order decides
  dev = pts.cuda()
  codes = morton_sort.morton_codes(dev, resolution).cpu().numpy().astype(np.uint64)
  want = omorton.morton_codes(pts.numpy(), resolution)
  assert codes.shape == (n,) and np.array_equal(codes, want)
  order = morton_sort.argsort(dev, resolution).cpu().numpy()
  assert np.array_equal(order, omorton.argsort(pts.numpy(), resolution))
  keep = morton_sort.argsort_dedup(dev, resolution).cpu().numpy()
  assert np.array_equal(keep, omorton.argsort_dedup(pts.numpy(), resolution))
  assert torch.equal(morton_sort.sort(dev, resolution).cpu(), pts[torch.from_numpy(order).long()])
  assert torch.equal(morton_sort.sort_dedup(dev, resolution).cpu(), pts[torch.from_numpy(keep).long()])


def test_morton_nan_and_empty():
  from taichi_splatting_amd.misc import morton_sort
  assert morton_sort.argsort(torch.empty(0, 3, device='cuda:0'), 0.1).shape == (0,)
  pts = torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.5, float('inf'), 0.5]], device='cuda:0')
  codes = morton_sort.morton_codes(pts, 0.25)
  assert codes.shape == (3,) and int(codes[0]) == 0 and int(codes[1]) == 0b111000000   # cell (4, 4, 4)


@pytest.mark.parametrize('n', [1, 63, 4096, 4097, 250_001])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('depth16', [False, True])
@pytest.mark.parametrize('ndc', [False, True])
def test_depth_argsort_equals_keys_then_stable_sort(n, dtype, depth16, ndc):
  """ms_depth_argsort (keys made inside the first radix pass) against ms_depth_sort_keys + a stable torch sort"""
  import ctypes
  from taichi_splatting_amd import _lib
  lib = _lib.load()
  torch.manual_seed(n)
  depth = (torch.rand(n, dtype=dtype) * (9.0 if ndc else 1.0) + (0.5 if ndc else 0.0)).to(DEV)
  depth[::7] = depth[0].clone()                           # ties: broken by index
  near, far = (0.25, 60.0) if ndc else (0.0, 0.0)
  stream = _lib.current_stream(torch.device(DEV))
  keys = torch.empty(n, dtype=torch.int32, device=DEV)
  vals = torch.empty(n, dtype=torch.int32, device=DEV)
  _lib.check(lib.ms_depth_sort_keys(depth.data_ptr(), n, int(depth16), near, far, keys.data_ptr(), vals.data_ptr(),
                                    _lib.dtype_code(dtype), stream), "keys")
  want_keys, want_order = torch.sort(keys.long() & 0xffffffff, stable=True)

  nb = ctypes.c_size_t(0)
  _lib.check(lib.ms_depth_argsort(None, n, int(depth16), near, far, _lib.dtype_code(dtype), None, None, None,
                                  ctypes.byref(nb), stream), "size")
  tmp = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=DEV)
  got_keys = torch.empty(n, dtype=torch.int32, device=DEV)
  got_order = torch.empty(n, dtype=torch.int32, device=DEV)
  _lib.check(lib.ms_depth_argsort(depth.data_ptr(), n, int(depth16), near, far, _lib.dtype_code(dtype),
                                  got_keys.data_ptr(), got_order.data_ptr(), tmp.data_ptr(), ctypes.byref(nb), stream), "argsort")
  assert torch.equal(got_order.long(), want_order)
  assert torch.equal(got_keys.long() & 0xffffffff, want_keys)


# ======================================================================================================================
# The paths of csrc/scan_sort.hip that random keys at a few sizes do not reach.  Cases and references:
# tests/primitive_cases.py (held to what they claim by tests/test_primitive_cases_host.py).  Exact integer work throughout.
# ======================================================================================================================
import ctypes

from taichi_splatting_amd import _lib
from tests import primitive_cases as pc


def _scan_abi(src, n, dst, total_host=None):
  """ms_exclusive_scan_i32 on raw pointers: src (n int32) -> dst (n + 1 int32)"""
  lib = _lib.load()
  stream = _lib.current_stream(torch.device(DEV))
  nb = ctypes.c_size_t(0)
  _lib.check(lib.ms_exclusive_scan_i32(None, n, None, None, None, ctypes.byref(nb), stream), "scan size")
  tmp = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=DEV)
  _lib.check(lib.ms_exclusive_scan_i32(src.data_ptr(), n, dst.data_ptr(), None if total_host is None else total_host.data_ptr(),
                                       tmp.data_ptr(), ctypes.byref(nb), stream), "scan")
  return tmp


def _want_scan(x):
  """(n + 1,) int64 exclusive scan with the total appended"""
  return torch.cat([torch.zeros(1, dtype=torch.int64, device=x.device), torch.cumsum(x.long(), 0)])


# ---- scan ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(pc.scan_switch_sizes()))
def test_full_cumsum_both_sides_of_the_spine_switch(name):
  """the last size of scan_downsweep_self_kernel, the first of scan_spine_kernel + scan_downsweep_kernel, and a spine
  whose last round is partial: every prefix and the total"""
  n = pc.scan_switch_sizes()[name]
  torch.manual_seed(n % 1000)
  x = torch.randint(0, 9, (n,), dtype=torch.int32, device=DEV)
  out, total = cuda_lib.full_cumsum(x)
  want = torch.cumsum(x, 0, dtype=torch.int64)
  assert int(want[-1]) < 2 ** 31
  assert out.shape[0] == n + 1 and int(out[0]) == 0
  assert torch.equal(out[1:], want.to(torch.int32))
  assert total == int(want[-1])


def test_full_cumsum_total_at_the_int32_limit():
  x = torch.from_numpy(pc.int32_limit_input()).to(DEV)
  out, total = cuda_lib.full_cumsum(x)
  want = _want_scan(x)
  assert int(want[-1]) == 2 ** 31 - 1 and total == 2 ** 31 - 1
  assert torch.equal(out.long(), want)


@pytest.mark.parametrize('n', pc.SCAN_SMALL_SIZES)
def test_scan_misaligned_and_in_place_through_the_c_abi(n):
  """in / out 4, 8 and 12 bytes off a 16-byte boundary (load_items / store_items leave their 128-bit path), and in == out"""
  torch.manual_seed(n)
  x = torch.randint(0, 9, (n,), dtype=torch.int32, device=DEV)
  want = _want_scan(x)
  for in_off, out_off in ((1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 3), (2, 2), (3, 1)):
    buf = torch.full((n + 8,), 77, dtype=torch.int32, device=DEV)
    obuf = torch.full((n + 9,), -5, dtype=torch.int32, device=DEV)
    assert buf.data_ptr() % 16 == 0 and obuf.data_ptr() % 16 == 0
    buf[in_off:in_off + n] = x
    _scan_abi(buf[in_off:], n, obuf[out_off:])
    assert torch.equal(obuf[out_off:out_off + n + 1].long(), want), f"in +{in_off}, out +{out_off}"
    assert bool((obuf[:out_off] == -5).all()) and bool((obuf[out_off + n + 1:] == -5).all()), "wrote outside out[0..n]"
    assert torch.equal(buf[in_off:in_off + n], x)
  for off in (0, 1, 2, 3):                                   # in place
    buf = torch.full((n + 9,), -5, dtype=torch.int32, device=DEV)
    buf[off:off + n] = x
    _scan_abi(buf[off:], n, buf[off:])
    assert torch.equal(buf[off:off + n + 1].long(), want), f"in place, +{off}"
    assert bool((buf[:off] == -5).all()) and bool((buf[off + n + 1:] == -5).all())


def test_full_cumsum_non_contiguous_input():
  torch.manual_seed(3)
  base = torch.randint(0, 9, (2 * (3 * pc.SCAN_TILE + 7),), dtype=torch.int32, device=DEV)
  x = base[::2]
  assert not x.is_contiguous()
  out, total = cuda_lib.full_cumsum(x)
  want = _want_scan(x)
  assert torch.equal(out.long(), want) and total == int(want[-1])


@pytest.mark.parametrize('n', [17, 3 * pc.SCAN_TILE + 7])
def test_scan_writes_the_total_to_a_pinned_host_word(n):
  torch.manual_seed(n)
  x = torch.randint(0, 9, (n,), dtype=torch.int32, device=DEV)
  out = torch.empty(n + 1, dtype=torch.int32, device=DEV)
  word = torch.full((1,), -1, dtype=torch.int32).pin_memory()
  _scan_abi(x, n, out, total_host=word)
  torch.cuda.current_stream().synchronize()
  assert int(word[0]) == int(x.long().sum()) == int(out[n])


# ---- radix sort ------------------------------------------------------------------------------------------------------

def _check_sort(keys, values, begin=0, end=None):
  """the WHOLE keys and the values come out in the order of a stable sort on key bits [begin, end)"""
  kd, vd = keys.to(DEV), values.to(DEV)
  bits = kd.element_size() * 8
  end = bits if end is None else end
  k_before, v_before = pc.as_signed(kd).clone(), vd.clone()
  ko, vo = cuda_lib.radix_sort_pairs(kd, vd, start_bit=begin, end_bit=end)
  perm = pc.stable_order(kd, begin, end)
  assert ko.dtype == keys.dtype and vo.dtype == torch.int32 and ko.shape == kd.shape
  assert torch.equal(pc.as_signed(ko), pc.as_signed(kd)[perm]), f"keys, bits [{begin}, {end})"
  assert torch.equal(vo, vd[perm]), f"values, bits [{begin}, {end})"
  assert torch.equal(pc.as_signed(kd), k_before) and torch.equal(vd, v_before), "inputs changed"
  return ko, vo


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('shape', pc.KEY_SHAPES)
def test_radix_sort_key_shapes(shape, dtype):
  """constant / sorted / reversed / alternating / one-bin / random keys at one block exactly, either side of it and
  several blocks, full width, with a payload that is no arange"""
  for n in pc.SORT_SIZES:
    _check_sort(pc.shaped_keys(shape, n, dtype, seed=n), pc.payload(n, seed=n))


@pytest.mark.parametrize('begin,end', pc.BIT_RANGES_32)
def test_radix_sort_bit_ranges_32(begin, end):
  n = 3 * pc.RS_TILE + 1
  keys, values = pc.random_keys(n, torch.int32, begin + end), pc.payload(n)
  ko, vo = _check_sort(keys, values, begin, end)
  if begin == end:                                           # the copy kernel
    assert torch.equal(ko.cpu(), keys) and torch.equal(vo.cpu(), values)


@pytest.mark.parametrize('begin,end', pc.BIT_RANGES_64)
def test_radix_sort_bit_ranges_64(begin, end):
  n = 3 * pc.RS_TILE + 1
  keys, values = pc.random_keys(n, torch.int64, begin + end), pc.payload(n)
  ko, vo = _check_sort(keys, values, begin, end)
  if begin == end:
    assert torch.equal(ko.cpu(), keys) and torch.equal(vo.cpu(), values)


def test_radix_sort_full_width_signed_int64():
  n = 2 * pc.RS_TILE + 1
  keys = pc.random_keys(n, torch.int64, 5)
  assert bool((keys < 0).any())
  ko, _ = _check_sort(keys, pc.payload(n))
  assert torch.equal(ko.cpu(), torch.sort(keys, stable=True)[0])


@pytest.mark.parametrize('begin,end', [(0, 16), (4, 12)])
def test_radix_sort_int16(begin, end):
  n = pc.RS_TILE + 1
  keys = pc.random_keys(n, torch.int16, 6)
  ko, _ = _check_sort(keys, pc.payload(n), begin, end)
  if (begin, end) == (0, 16):
    assert torch.equal(ko.cpu(), torch.sort(keys, stable=True)[0])


@pytest.mark.parametrize('dtype,begin,end', [(torch.uint32, 0, 32), (torch.uint32, 5, 19), (torch.uint64, 0, 64),
                                             (torch.uint64, 32, 46)])
def test_radix_sort_unsigned_dtypes(dtype, begin, end):
  n = 2 * pc.RS_TILE + 1
  keys = pc.random_keys(n, dtype, 7)
  assert keys.dtype == dtype
  _check_sort(keys, pc.payload(n), begin, end)


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_radix_sort_non_contiguous_inputs(dtype):
  n = pc.RS_TILE + 1
  keys = pc.random_keys(2 * n, dtype, 8).to(DEV)[::2]
  values = pc.payload(3 * n).to(DEV)[::3]
  assert not keys.is_contiguous() and not values.is_contiguous()
  _check_sort(keys, values)


@pytest.mark.parametrize('dtype,begin,end', [(torch.int32, 0, 32), (torch.int64, 32, 46)])
def test_radix_sort_second_round_of_the_row_scan(dtype, begin, end):
  """more per-block counts per digit than one round of row_scan_body holds: the carry between its rounds"""
  n = pc.row_scan_second_round_size()
  gen = torch.Generator(device=DEV).manual_seed(end)
  lo, hi = (-(1 << 31), (1 << 31) - 1) if dtype == torch.int32 else (-(1 << 63), (1 << 63) - 1)
  keys = torch.randint(lo, hi, (n,), dtype=dtype, device=DEV, generator=gen)
  values = torch.randint(-50, 50, (n,), dtype=torch.int32, device=DEV, generator=gen)
  ko, vo = cuda_lib.radix_sort_pairs(keys, values, start_bit=begin, end_bit=end)
  perm = pc.stable_order(keys, begin, end)
  assert torch.equal(ko, keys[perm])
  assert torch.equal(vo, values[perm])


# ---- segmented sort, ranges ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [torch.int32, torch.int16])
def test_segmented_sort_pairs_segments_gaps_and_order(dtype):
  """negative keys, segment lengths 0 / 1 / 2 / 256 / 257 / 3000 listed out of order, gaps copied through unchanged"""
  n, starts, ends = pc.segments_with_gaps()
  gen = torch.Generator().manual_seed(11)
  keys = torch.randint(-40, 40, (n,), dtype=torch.int64, generator=gen).to(dtype)
  values = pc.payload(n)
  want_k, want_v = pc.segmented_reference(keys, values, starts, ends)
  ko, vo = cuda_lib.segmented_sort_pairs(keys.to(DEV), values.to(DEV), torch.tensor(starts, dtype=torch.int64, device=DEV),
                                         torch.tensor(ends, dtype=torch.int64, device=DEV))
  assert ko.dtype == dtype
  assert torch.equal(ko.cpu(), want_k) and torch.equal(vo.cpu(), want_v)


def test_segmented_sort_pairs_no_segments_and_no_elements():
  keys = torch.tensor([3, -1, 2], dtype=torch.int32, device=DEV)
  values = torch.tensor([7, 7, -9], dtype=torch.int32, device=DEV)
  none = torch.empty(0, dtype=torch.int64, device=DEV)
  ko, vo = cuda_lib.segmented_sort_pairs(keys[:0], values[:0], none, none)
  assert ko.shape == (0,) and vo.shape == (0,)
  one = torch.zeros(1, dtype=torch.int64, device=DEV)
  ko, vo = cuda_lib.segmented_sort_pairs(keys[:0], values[:0], one, one)
  assert ko.shape == (0,) and vo.shape == (0,)
  # zero segments over three elements: every element lies outside every segment and is copied through
  ko, vo = cuda_lib.segmented_sort_pairs(keys, values, none, none)
  assert ko.tolist() == [3, -1, 2] and vo.tolist() == [7, 7, -9]
  assert keys.tolist() == [3, -1, 2] and values.tolist() == [7, 7, -9]


def _find_ranges(keys_np, key_bytes, shift, num_tiles):
  lib = _lib.load()
  signed = keys_np.view(np.int32 if key_bytes == 4 else np.int64)
  keys = torch.from_numpy(signed.copy()).to(DEV)
  out = torch.full((max(num_tiles, 1), 2), -7, dtype=torch.int32, device=DEV)
  _lib.check(lib.ms_find_ranges(keys.data_ptr(), keys.shape[0], key_bytes, shift, num_tiles, out.data_ptr(),
                                _lib.current_stream(torch.device(DEV))), "find_ranges")
  return out[:num_tiles].cpu().numpy()


@pytest.mark.parametrize('key_bytes', [4, 8])
@pytest.mark.parametrize('shift', [0, 16, 32])
def test_find_ranges_against_bincount(key_bytes, shift):
  """ms_find_ranges itself: one tile only, every key its own tile, runs with empty tiles in between and ids >= num_tiles
  (ignored), at k around one 256-thread block.  A shift by the whole width of a 4-byte key leaves tile 0."""
  utype = np.uint32 if key_bytes == 4 else np.uint64
  rng = np.random.default_rng(shift + key_bytes)
  whole = shift >= 8 * key_bytes
  low_bits = min(shift, 8 * key_bytes)
  id_limit = 1 << min(8 * key_bytes - shift, 20) if not whole else 1

  def keys_of(ids):
    low = rng.integers(0, 1 << low_bits, size=ids.shape[0], dtype=np.uint64) if low_bits else np.zeros(ids.shape[0], dtype=np.uint64)
    keys = np.sort(((ids.astype(np.uint64) << np.uint64(shift)) if not whole else np.zeros_like(low)) | low)
    return keys.astype(utype)

  for k in (1, 255, 256, 257):
    cases = {
      'one_tile': (np.full(k, 3 % id_limit), 7),
      'own_tile': (np.arange(k) % id_limit, k),
      'own_tile_some_ignored': (np.arange(k) % id_limit, max(k - 2, 1)),
      'runs': (np.sort(rng.integers(0, min(44, id_limit), size=k)), 40),
    }
    for name, (ids, num_tiles) in cases.items():
      ids = np.sort(np.asarray(ids, dtype=np.int64))
      got = _find_ranges(keys_of(ids), key_bytes, shift, num_tiles)
      assert np.array_equal(got, pc.ranges_reference(ids, num_tiles)), f"{name}, k {k}"
  assert _find_ranges(np.zeros(0, dtype=utype), key_bytes, shift, 5).tolist() == [[0, 0]] * 5
  for bad in (-1, 8 * key_bytes + 1):
    with pytest.raises(ValueError, match="tile_shift"):
      _find_ranges(np.zeros(4, dtype=utype), key_bytes, bad, 5)
