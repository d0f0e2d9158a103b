"""Shared by tests/test_primitive_cases_host.py (CPU) and the GPU tests of the integer primitives of
``csrc/scan_sort.hip`` (tests/test_gpu_primitives.py, tests/test_gpu_frame_primitives.py): the case tables and their pure
torch / numpy references.  Everything here is exact integer work; no tolerance appears anywhere.

* sizes that are derived from the kernels' own constants (parsed out of the source), so that a changed threshold moves
  the cases instead of silently un-covering a path;
* depth-key sets whose bytes vary in exactly a chosen subset: the 16 routes of the adaptive depth pre-sort;
* splats that overlap exactly one tile, so that a frame's overlap total K equals its gaussian count and a test can
  choose K to the element, and the expected tile lists of such a frame;
* the ordering a radix sort on key bits [begin, end) must produce, and key sets of the shapes that stress its ranking.

The CPU test proves that the cases are what they claim before any kernel is looked at."""
import re
from pathlib import Path

import numpy as np
import torch

SOURCE = Path(__file__).resolve().parents[1] / 'taichi_splatting_amd' / 'csrc' / 'scan_sort.hip'


# ---- sizes that follow the code -----------------------------------------------------------------------------------------

def constants(text=None):
  """the integer constants of scan_sort.hip the big cases depend on, plus the two tile sizes derived from them"""
  text = SOURCE.read_text() if text is None else text
  out = {}
  for name in ('SCAN_THREADS', 'SCAN_ITEMS', 'SCAN_SELF_MAX_BLOCKS', 'RS_THREADS', 'RS_ROUNDS'):
    m = re.findall(r'constexpr\s+(?:int|int64_t)\s+%s\s*=\s*(\d+)\s*;' % name, text)
    assert len(m) == 1, f"{name}: expected one definition in {SOURCE.name}, found {len(m)}"
    out[name] = int(m[0])
  # the two products are spelled out in the source: hold the source to that spelling
  assert re.search(r'constexpr\s+int\s+SCAN_TILE\s*=\s*SCAN_THREADS\s*\*\s*SCAN_ITEMS\s*;', text), "SCAN_TILE is no longer SCAN_THREADS * SCAN_ITEMS"
  assert re.search(r'constexpr\s+int\s+RS_TILE\s*=\s*RS_THREADS\s*\*\s*RS_ROUNDS\s*;', text), "RS_TILE is no longer RS_THREADS * RS_ROUNDS"
  out['SCAN_TILE'] = out['SCAN_THREADS'] * out['SCAN_ITEMS']
  out['RS_TILE'] = out['RS_THREADS'] * out['RS_ROUNDS']
  return out


C = constants()
SCAN_TILE, RS_TILE = C['SCAN_TILE'], C['RS_TILE']


def div_up(a, b):
  return (a + b - 1) // b


def scan_blocks(n):
  """tiles of exclusive_scan_i32 at n elements"""
  return div_up(n, SCAN_TILE)


def radix_blocks(n):
  """blocks of one radix pass at n keys = entries of one digit's row of the histogram"""
  return div_up(n, RS_TILE)


def scan_switch_sizes(c=None):
  """{name: n} on both sides of the switch from the self-summing downsweep to spine + downsweep, and a spine whose last
  round of SCAN_THREADS tile sums is partial"""
  c = C if c is None else c
  b, t = c['SCAN_SELF_MAX_BLOCKS'], c['SCAN_TILE']
  return {'last_self': b * t, 'first_spine': b * t + 1, 'spine_partial_round': (b + 256) * t + 4097}


def row_scan_second_round_size(c=None):
  """keys at which a digit's row of per-block counts (one entry per RS_TILE keys) no longer fits one round of SCAN_TILE
  entries of row_scan_body: the carry between rounds is used"""
  c = C if c is None else c
  return c['SCAN_TILE'] * c['RS_TILE'] + 4097


SCAN_SMALL_SIZES = (15, 16, 17, SCAN_TILE - 1, SCAN_TILE + 1, 3 * SCAN_TILE + 7)
INT32_LIMIT_N = 3 * SCAN_TILE + 5


def int32_limit_input():
  """int32 vector of INT32_LIMIT_N entries, zero but for six, whose total is exactly 2^31 - 1"""
  x = np.zeros(INT32_LIMIT_N, dtype=np.int64)
  x[0] = 1
  x[SCAN_TILE - 1] = 1 << 29
  x[SCAN_TILE] = 1 << 29
  x[2 * SCAN_TILE + 3] = (1 << 30) - 2 - 7
  x[3 * SCAN_TILE] = 3
  x[INT32_LIMIT_N - 1] = 4
  return x.astype(np.int32)


# ---- depth keys with a chosen vary mask ---------------------------------------------------------------------------------

VARY_SIZES = (1, 63, RS_TILE - 1, RS_TILE, RS_TILE + 1, 3 * RS_TILE + 5)
# values a varying byte takes (three each: many ties) and the value of a constant byte; the top byte stays in 0x30..0x3f,
# so every key is the bit pattern of a positive finite float32 (2^-31 .. 2) and never the culled key 0xffffffff
_VARYING = ((0x01, 0xfe, 0x80), (0x02, 0xfd, 0x7f), (0x00, 0xff, 0x81), (0x30, 0x3f, 0x38))
_CONSTANT = (0x5a, 0xa5, 0x33, 0x3c)


def vary_keys(mask, n, seed=0):
  """n uint32 keys whose bytes differ, over the set, in exactly the bytes of ``mask`` (bit b = byte b), for n >= 2;
  in storage order they are unsorted and full of ties"""
  rng = np.random.default_rng(1000 * mask + seed)
  keys = np.zeros(n, dtype=np.uint32)
  for b in range(4):
    if (mask >> b) & 1:
      pick = rng.integers(0, 3, size=n)
      pick[:2] = (1, 0)[:n]                 # two different values for certain, the larger one first
      byte = np.asarray(_VARYING[b], dtype=np.uint32)[pick]
    else:
      byte = np.full(n, _CONSTANT[b], dtype=np.uint32)
    keys |= byte << np.uint32(8 * b)
  return keys


def vary_mask_of(keys):
  """4-bit mask of the bytes in which the keys differ: OR xor AND, as the kernels compute it"""
  keys = np.asarray(keys, dtype=np.uint32)
  diff = int(np.bitwise_or.reduce(keys) ^ np.bitwise_and.reduce(keys))
  return sum(1 << b for b in range(4) if (diff >> (8 * b)) & 0xff)


DEPTH16_KINDS = {'constant': 0b00, 'low_byte': 0b01, 'high_byte': 0b10, 'both_bytes': 0b11}


def depth16_depths(kind, n, seed=0):
  """float32 depths (q + 0.5) / 65535 whose 16-bit keys q vary in the bytes DEPTH16_KINDS[kind] only"""
  rng = np.random.default_rng(seed + 7)
  mask = DEPTH16_KINDS[kind]
  lo = np.asarray((0x03, 0xfc, 0x80))[rng.integers(0, 3, size=n)] if mask & 1 else np.full(n, 0x34)
  hi = np.asarray((0x00, 0xfe, 0x41))[rng.integers(0, 3, size=n)] if mask & 2 else np.full(n, 0x12)
  if n >= 2:
    if mask & 1: lo[:2] = (0xfc, 0x03)
    if mask & 2: hi[:2] = (0xfe, 0x00)
  q = hi.astype(np.int64) * 256 + lo.astype(np.int64)
  return ((q.astype(np.float64) + 0.5) / 65535.0).astype(np.float32), q.astype(np.uint32)


# ---- one-tile splats: K = n ----------------------------------------------------------------------------------------------

# name -> (tiles wide, tiles high, tile size); tile bits and radix passes of the tile sort in the comment
GRIDS = {
  '13x7_t16': (13, 7, 16),       # 91 tiles: 7 bits, one pass
  '23x13_t8': (23, 13, 8),       # 299 tiles: 9 bits = 5 + 4
  '40x13_t8': (40, 13, 8),       # 520 tiles: 10 bits = 5 + 5
  '5x3_t32': (5, 3, 32),         # 15 tiles: 4 bits
}
BIG_GRID = (300, 220, 8)         # 66 000 tiles: 17 bits = 6 + 6 + 5
CHOSEN_K = (1, 2, 3, 4, 5, 126, 127, 128, 129, 130, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 8195)
ASSIGNMENTS = ('first_tile', 'last_tile', 'round_robin', 'random_third')
CAPACITY_K = (1025, 4097)
FEW_DEPTHS = np.asarray([0.25, 0.5, 0.75, 0.7500001], dtype=np.float32)


def tile_bits(num_tiles):
  bits = 1
  while (1 << bits) < num_tiles:
    bits += 1
  return bits


def image_size(grid):
  """an image of that many tiles whose last tile column and row are partial"""
  tw, th, ts = grid
  return (tw * ts - ts // 4, th * ts - ts // 4)


def tile_assignment(kind, n, num_tiles, seed=0):
  """(n,) int64 tile of every splat"""
  if kind == 'first_tile':
    return np.zeros(n, dtype=np.int64)
  if kind == 'last_tile':
    return np.full(n, num_tiles - 1, dtype=np.int64)
  if kind == 'round_robin':
    return np.arange(n, dtype=np.int64) % num_tiles
  assert kind == 'random_third'
  rng = np.random.default_rng(seed + n)
  used = np.sort(rng.choice(num_tiles, size=max(num_tiles // 3, 1), replace=False))     # empty tiles in between
  return used[rng.integers(0, used.shape[0], size=n)].astype(np.int64)


def one_tile_splats(tiles, grid):
  """(n, 7) float32 packed 2D gaussians [tile centre, axis (1, 0), sigma (0.5, 0.5), alpha 0.5]: at the default alpha
  threshold their extent is 1.56 pixels, inside any tile of 8 pixels or more"""
  tw, th, ts = grid
  tiles = np.asarray(tiles, dtype=np.int64)
  p = np.zeros((tiles.shape[0], 7), dtype=np.float32)
  p[:, 0] = (tiles % tw) * ts + ts / 2
  p[:, 1] = (tiles // tw) * ts + ts / 2
  p[:, 2], p[:, 3] = 1.0, 0.0
  p[:, 4:6] = 0.5
  p[:, 6] = 0.5
  return p


def few_depths(n, seed=0):
  """(n,) float32 depths of four distinct values, two of them one ulp-scale step apart"""
  return FEW_DEPTHS[np.random.default_rng(seed + 31 * n).integers(0, FEW_DEPTHS.shape[0], size=n)]


def expected_lists(tiles, key_bits, num_tiles):
  """(overlap_to_point (n,) int32, tile_ranges (num_tiles, 2) int32) of a frame of one-tile splats: order (tile, depth
  key bits, point index); ranges from the tiles' counts, [0, 0) for an empty tile"""
  tiles = np.asarray(tiles, dtype=np.int64)
  n = tiles.shape[0]
  order = np.lexsort((np.arange(n), np.asarray(key_bits, dtype=np.uint64), tiles))
  counts = np.bincount(tiles, minlength=num_tiles).astype(np.int64)
  end = np.cumsum(counts)
  ranges = np.stack([end - counts, end], axis=1)
  ranges[counts == 0] = 0
  return order.astype(np.int32), ranges.astype(np.int32)


# ---- radix sort: the order it must produce -------------------------------------------------------------------------------

SIGNED = (torch.int16, torch.int32, torch.int64)
_SIGNED_OF_SIZE = {2: torch.int16, 4: torch.int32, 8: torch.int64}
SORT_SIZES = (RS_TILE - 1, RS_TILE, RS_TILE + 1, 2 * RS_TILE, 3 * RS_TILE + 1)
KEY_SHAPES = ('constant', 'ascending', 'descending', 'alternating', 'one_digit', 'random')
BIT_RANGES_32 = ((0, 1), (3, 4), (5, 19), (0, 9), (0, 17), (7, 32), (12, 12))
BIT_RANGES_64 = ((28, 37), (32, 46), (32, 49), (0, 33), (1, 64), (40, 40))


def as_signed(keys):
  """the same bits as a signed tensor (torch indexes and compares those on every device)"""
  return keys if keys.dtype in SIGNED else keys.view(_SIGNED_OF_SIZE[keys.element_size()])


def window_digits(keys, begin, end):
  """int64 tensor whose ascending order is the order ``radix_sort_pairs(keys, start_bit=begin, end_bit=end)`` documents:
  the unsigned value of key bits [begin, end); for a signed dtype whose window ends at the sign bit, that bit inverted
  (negative keys first: the signed order of key >> begin, what a full-width sort of signed keys means)"""
  signed = keys.dtype in SIGNED
  bits = keys.element_size() * 8
  assert 0 <= begin <= end <= bits
  k = as_signed(keys).to(torch.int64)
  width = end - begin
  if width == 0:
    return torch.zeros_like(k)
  if width == 64:
    return k if signed else k ^ (-(1 << 63))
  if bits < 64:
    k = k & ((1 << bits) - 1)
  d = (k >> begin) & ((1 << width) - 1)
  if signed and end == bits:
    d = d ^ (1 << (width - 1))
  return d


def stable_order(keys, begin, end):
  """the permutation a stable sort on key bits [begin, end) applies"""
  return torch.sort(window_digits(keys, begin, end), stable=True)[1]


def random_keys(n, dtype, seed):
  """n keys of every bit pattern of the dtype (both signs, random high bits), a third of them from 17 values: ties"""
  gen = torch.Generator().manual_seed(seed)
  raw = torch.randint(-(1 << 63), (1 << 63) - 1, (n,), dtype=torch.int64, generator=gen)
  few = torch.randint(-(1 << 63), (1 << 63) - 1, (17,), dtype=torch.int64, generator=gen)
  raw[::3] = few[torch.randint(0, 17, (raw[::3].shape[0],), generator=gen)]
  size = torch.empty((), dtype=dtype).element_size()
  signed = raw.to(_SIGNED_OF_SIZE[size]) if size == 8 else (raw >> (64 - 8 * size)).to(_SIGNED_OF_SIZE[size])
  return signed if dtype in SIGNED else signed.view(dtype)


def shaped_keys(shape, n, dtype, seed=0):
  """int32 / int64 keys of one of KEY_SHAPES; both halves of a 64-bit key vary wherever the shape lets anything vary"""
  assert dtype in (torch.int32, torch.int64)
  wide = dtype == torch.int64
  i = torch.arange(n, dtype=torch.int64)
  if shape == 'constant':
    k = torch.full((n,), 0x5a5a5a5a5a5a5a5a if wide else 0x5a5a5a5a, dtype=torch.int64)
  elif shape in ('ascending', 'descending'):
    k = (i - n // 2) * (0x1000010000019 if wide else 0x10019)    # negative to positive, every byte of the key moves
    if shape == 'descending':
      k = k.flip(0)
  elif shape == 'alternating':                              # neighbouring lanes hold different digits in every pass
    a, b = (0x0123456789abcdef, -0x0123456789abcdef) if wide else (0x01234567, -0x01234567)
    k = torch.where(i % 2 == 0, torch.tensor(a), torch.tensor(b))
  elif shape == 'one_digit':                                # all but 1 in 1000 keys are one value: one bin takes the block
    k = torch.full((n,), 0x3c3c3c3c3c3c3c3c if wide else 0x3c3c3c3c, dtype=torch.int64)
    odd = torch.arange(7, n, 1000)
    k[odd] = random_keys(odd.shape[0], dtype, seed).to(torch.int64)
  else:
    assert shape == 'random'
    k = random_keys(n, dtype, seed).to(torch.int64)
  return k.to(dtype)


def payload(n, seed=0):
  """int32 values with negatives and duplicates"""
  return torch.randint(-50, 50, (n,), dtype=torch.int32, generator=torch.Generator().manual_seed(seed + 99))


# ---- segments and ranges -------------------------------------------------------------------------------------------------

SEGMENT_LENGTHS = (0, 1, 2, 256, 257, 3000)


def segments_with_gaps():
  """(n, starts, ends): segments of SEGMENT_LENGTHS, listed out of order, with gaps of 0, 1 or 5 elements around them"""
  starts, ends, at = [], [], 3
  for length, gap in zip(SEGMENT_LENGTHS, (0, 1, 5, 0, 5, 1)):
    starts.append(at)
    ends.append(at + length)
    at += length + gap
  order = [4, 0, 5, 2, 1, 3]
  return at + 2, [starts[j] for j in order], [ends[j] for j in order]


def segmented_reference(keys, values, starts, ends):
  """keys / values (CPU tensors) with every segment stably sorted by key and everything else left where it was"""
  ko, vo = keys.clone(), values.clone()
  for s, e in zip(starts, ends):
    order = torch.sort(keys[s:e].to(torch.int64), stable=True)[1]
    ko[s:e], vo[s:e] = keys[s:e][order], values[s:e][order]
  return ko, vo


def ranges_reference(tile_ids, num_tiles):
  """(num_tiles, 2) int32 [first, last + 1) of every tile id < num_tiles in the SORTED id list, [0, 0) where absent"""
  ids = np.asarray(tile_ids, dtype=np.int64)
  assert np.all(ids[1:] >= ids[:-1])
  counts_all = np.bincount(ids, minlength=num_tiles).astype(np.int64)
  end = np.cumsum(counts_all)
  ranges = np.stack([end - counts_all, end], axis=1)[:num_tiles]
  ranges[counts_all[:num_tiles] == 0] = 0
  return ranges.astype(np.int32)
