"""CPU: the cases of tests/primitive_cases.py are what they claim, before any kernel is looked at.  This test alone fails
when a case stops reaching its path: a changed threshold constant, a splat that touches two tiles, a key set with the wrong
vary mask."""
import numpy as np
import pytest
import torch

from oracle import mapper as omap
from tests import primitive_cases as pc

ALPHA_THRESHOLD = 1. / 255.


# ---- sizes follow the code -----------------------------------------------------------------------------------------------

def test_constants_are_parsed_from_the_source():
  c = pc.constants()
  assert c['SCAN_TILE'] == c['SCAN_THREADS'] * c['SCAN_ITEMS'] and c['RS_TILE'] == c['RS_THREADS'] * c['RS_ROUNDS']
  # a changed constant moves the derived sizes
  text = pc.SOURCE.read_text().replace('SCAN_SELF_MAX_BLOCKS = %d;' % c['SCAN_SELF_MAX_BLOCKS'], 'SCAN_SELF_MAX_BLOCKS = 100;')
  moved = pc.constants(text)
  assert moved['SCAN_SELF_MAX_BLOCKS'] == 100
  assert pc.scan_switch_sizes(moved)['first_spine'] == 100 * c['SCAN_TILE'] + 1
  with pytest.raises(AssertionError):
    pc.constants(text.replace('constexpr int RS_ROUNDS', 'constexpr int RS_ITEMS'))


def test_scan_sizes_land_on_the_intended_side_of_the_switch():
  c, sizes = pc.C, pc.scan_switch_sizes()
  limit = c['SCAN_SELF_MAX_BLOCKS']
  assert pc.scan_blocks(sizes['last_self']) == limit                      # the largest scan of the self-summing downsweep
  assert pc.scan_blocks(sizes['first_spine']) == limit + 1                # one element more: spine + downsweep
  blocks = pc.scan_blocks(sizes['spine_partial_round'])
  assert blocks > limit
  # the spine walks SCAN_THREADS tile sums per round: more than one round, the last one partial, as is the last tile
  assert blocks > c['SCAN_THREADS'] and blocks % c['SCAN_THREADS'] != 0
  assert sizes['spine_partial_round'] % c['SCAN_TILE'] != 0
  for n in sizes.values():
    assert n < 2 ** 31 and 8 * n < 2 ** 31                                # values 0..8: the total stays an int32
  # the small sizes: below, at and above one thread's items and one tile, and several tiles with a tail
  assert set(pc.SCAN_SMALL_SIZES) >= {c['SCAN_ITEMS'] - 1, c['SCAN_ITEMS'], c['SCAN_ITEMS'] + 1, c['SCAN_TILE'] - 1, c['SCAN_TILE'] + 1}
  assert pc.scan_blocks(max(pc.SCAN_SMALL_SIZES)) == 4


def test_row_scan_size_needs_a_second_round():
  c = pc.C
  n = pc.row_scan_second_round_size()
  # row_scan_body scans SCAN_TILE per-block counts per round
  assert pc.radix_blocks(n) > c['SCAN_TILE'] and pc.radix_blocks(n - 4097 - 1) <= c['SCAN_TILE']
  assert pc.radix_blocks(n) % c['SCAN_TILE'] not in (0, c['SCAN_TILE'])   # a partial second round
  assert n % c['RS_TILE'] != 0 and n < 2 ** 31
  assert pc.radix_blocks(max(pc.SORT_SIZES)) == 4 and pc.radix_blocks(max(pc.VARY_SIZES)) == 4
  assert {c['RS_TILE'] - 1, c['RS_TILE'], c['RS_TILE'] + 1} <= set(pc.SORT_SIZES) and {c['RS_TILE'] - 1, c['RS_TILE'], c['RS_TILE'] + 1} <= set(pc.VARY_SIZES)


def test_int32_limit_input():
  x = pc.int32_limit_input().astype(np.int64)
  assert x.shape[0] == 3 * pc.SCAN_TILE + 5 and (x >= 0).all()
  assert int(x.sum()) == 2 ** 31 - 1
  assert np.count_nonzero(x) >= 4 and len({i // pc.SCAN_TILE for i in np.flatnonzero(x)}) == 4     # in every tile


# ---- vary masks ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mask', range(16))
def test_key_sets_have_the_intended_vary_mask(mask):
  for n in pc.VARY_SIZES:
    keys = pc.vary_keys(mask, n)
    assert keys.dtype == np.uint32 and keys.shape == (n,)
    assert pc.vary_mask_of(keys) == (mask if n >= 2 else 0), f"mask {mask:04b}, n {n}"
    top = keys >> 24
    assert ((top >= 0x30) & (top <= 0x3f)).all()
    as_float = keys.view(np.float32)
    assert np.isfinite(as_float).all() and (as_float > 0).all()
    if n >= 63:
      assert np.unique(keys).shape[0] <= 81 < n or n == 63                # ties
      if mask:
        assert not np.array_equal(np.sort(keys, kind='stable'), keys)     # the sort has work to do
    # float bits of the depth are the key: the round trip through float32 keeps them
    assert np.array_equal(omap.depth_key_bits(as_float, False), keys.astype(np.uint64))


@pytest.mark.parametrize('kind', list(pc.DEPTH16_KINDS))
def test_depth16_sets_vary_in_the_intended_bytes(kind):
  for n in pc.VARY_SIZES:
    depth, q = pc.depth16_depths(kind, n)
    keys = omap.depth_key_bits(depth, True)
    assert np.array_equal(keys, q.astype(np.uint64)), "a depth (q + 0.5) / 65535 quantises to q"
    assert pc.vary_mask_of(keys.astype(np.uint32)) == (pc.DEPTH16_KINDS[kind] if n >= 2 else 0)


# ---- one-tile splats -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('grid', ['13x7_t16', '23x13_t8', '5x3_t32'])
def test_splats_overlap_exactly_one_tile_and_helper_agrees_with_oracle(grid):
  g = pc.GRIDS[grid]
  tw, th, ts = g
  n, num_tiles = 1031, tw * th
  tiles = pc.tile_assignment('round_robin', n, num_tiles)
  assert tiles[0] == 0 and (tiles == num_tiles - 1).any()
  points = pc.one_tile_splats(tiles, g)
  pid, tx, ty = omap.overlaps(points, pc.image_size(g), ts, ALPHA_THRESHOLD)
  assert np.array_equal(pid, np.arange(n)), "exactly one overlap per splat: K = n"
  assert np.array_equal(tx + ty * tw, tiles)
  depth = pc.few_depths(n)
  assert np.unique(depth).shape[0] == 4
  o2p, ranges, counts = omap.map_to_tiles(points, depth, pc.image_size(g), ts, ALPHA_THRESHOLD)
  want_o2p, want_ranges = pc.expected_lists(tiles, omap.depth_key_bits(depth, False), num_tiles)
  assert (counts == 1).all()
  assert np.array_equal(o2p, want_o2p) and np.array_equal(ranges.reshape(-1, 2), want_ranges)


@pytest.mark.parametrize('kind', pc.ASSIGNMENTS)
def test_assignments_and_helper_agree_with_oracle(kind):
  g = pc.GRIDS['40x13_t8']
  tw, th, ts = g
  num_tiles = tw * th
  for n in (1, 5, 513):
    tiles = pc.tile_assignment(kind, n, num_tiles)
    assert tiles.min() >= 0 and tiles.max() < num_tiles
    if kind == 'random_third':
      assert np.unique(pc.tile_assignment(kind, 8195, num_tiles)).shape[0] <= num_tiles // 3
    points, depth = pc.one_tile_splats(tiles, g), pc.few_depths(n)
    o2p, ranges, _ = omap.map_to_tiles(points, depth, pc.image_size(g), ts, ALPHA_THRESHOLD)
    want_o2p, want_ranges = pc.expected_lists(tiles, omap.depth_key_bits(depth, False), num_tiles)
    assert np.array_equal(o2p, want_o2p) and np.array_equal(ranges.reshape(-1, 2), want_ranges)
    empty = np.bincount(tiles, minlength=num_tiles) == 0
    assert (want_ranges[empty] == 0).all()


def test_grids_have_the_intended_tile_bits():
  bits = {name: pc.tile_bits(tw * th) for name, (tw, th, _) in pc.GRIDS.items()}
  assert bits == {'13x7_t16': 7, '23x13_t8': 9, '40x13_t8': 10, '5x3_t32': 4}
  tw, th, ts = pc.BIG_GRID
  assert tw * th > 65536 and pc.tile_bits(tw * th) == 17 and ts == 8
  # the big grid's splats sit in one tile each as well (first, last and a sample in between)
  tiles = np.asarray([0, 1, tw - 1, tw, 65535, 65536, tw * th - 1])
  pid, tx, ty = omap.overlaps(pc.one_tile_splats(tiles, pc.BIG_GRID), pc.image_size(pc.BIG_GRID), ts, ALPHA_THRESHOLD)
  assert np.array_equal(pid, np.arange(tiles.shape[0])) and np.array_equal(tx + ty * tw, tiles)
  # chosen K: around the keys-per-thread, wave (128 keys of the u64 kernel) and block (512 / 1024 keys) boundaries
  for edge in (4, 128, 512, 1024, 4096):
    assert {edge - 1, edge, edge + 1} <= set(pc.CHOSEN_K)


# ---- radix order ---------------------------------------------------------------------------------------------------------

def test_window_digits_is_the_documented_order():
  k = torch.tensor([5, -3, 0, -(1 << 31), (1 << 31) - 1, -1], dtype=torch.int32)
  assert torch.equal(k[pc.stable_order(k, 0, 32)], torch.sort(k, stable=True)[0])              # full width: signed
  assert pc.window_digits(k, 3, 4).tolist() == [0, 1, 0, 0, 1, 1]                              # a window: unsigned bits
  assert pc.window_digits(k, 12, 12).tolist() == [0] * 6                                       # empty: nothing moves
  assert torch.equal(k[pc.stable_order(k, 7, 32)] >> 7, torch.sort(k >> 7, stable=True)[0])    # ends at the sign bit: signed
  u = k.view(torch.uint32)
  assert pc.window_digits(u, 0, 32).tolist() == [5, 2 ** 32 - 3, 0, 2 ** 31, 2 ** 31 - 1, 2 ** 32 - 1]
  q = torch.tensor([1, -1, -(1 << 63), (1 << 63) - 1, 0], dtype=torch.int64)
  assert q[pc.stable_order(q, 0, 64)].tolist() == sorted(q.tolist())
  assert q[pc.stable_order(q.view(torch.uint64), 0, 64)].tolist() == [0, 1, (1 << 63) - 1, -(1 << 63), -1]
  assert q[pc.stable_order(q, 1, 64)].tolist() == [-(1 << 63), -1, 1, 0, (1 << 63) - 1]         # (q >> 1) signed, stable
  assert pc.window_digits(q, 32, 46).tolist() == [0, (1 << 14) - 1, 0, (1 << 14) - 1, 0]
  s = torch.tensor([-2, 1, -32768, 32767], dtype=torch.int16)
  assert s[pc.stable_order(s, 0, 16)].tolist() == [-32768, -2, 1, 32767]
  assert pc.window_digits(s, 4, 12).tolist() == [0xff, 0, 0, 0xff]


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_key_shapes_are_what_they_claim(dtype):
  n = 3 * pc.RS_TILE + 1
  bits = 32 if dtype == torch.int32 else 64
  keys = {shape: pc.shaped_keys(shape, n, dtype) for shape in pc.KEY_SHAPES}
  assert all(k.dtype == dtype and k.shape == (n,) for k in keys.values())
  assert keys['constant'].unique().shape[0] == 1
  asc, desc = keys['ascending'].long(), keys['descending'].long()
  assert (asc[1:] > asc[:-1]).all() and (desc[1:] < desc[:-1]).all() and asc[0] < 0 < asc[-1]
  alt = keys['alternating']
  assert alt.unique().shape[0] == 2 and (alt[0::2] == alt[0]).all() and (alt[1::2] == alt[1]).all()
  for b in range(0, bits, 8):                                  # the two values differ in every digit
    assert ((int(alt[0]) >> b) & 0xff) != ((int(alt[1]) >> b) & 0xff)
  one = keys['one_digit']
  common = one.mode().values
  assert 0 < int((one != common).sum()) <= n // 1000 + 1
  rnd = keys['random'].long()
  assert (rnd < 0).any() and (rnd > 0).any() and rnd.unique().shape[0] < n
  diff = 0
  for v in (rnd, asc):                                         # every byte of the key takes part
    diff = int(np.bitwise_or.reduce(v.numpy()) ^ np.bitwise_and.reduce(v.numpy())) & ((1 << bits) - 1)
    assert all((diff >> b) & 0xff for b in range(0, bits, 8))
  v = pc.payload(n)
  assert (v < 0).any() and v.unique().shape[0] < n and v.dtype == torch.int32
  for dt in (torch.int16, torch.uint32, torch.uint64):
    r = pc.random_keys(1000, dt, 0)
    assert r.dtype == dt and (pc.as_signed(r) < 0).any()
  for begin, end in pc.BIT_RANGES_64:                          # the 64-bit windows see bits that vary
    if end > begin:
      assert pc.window_digits(keys['random'] if dtype == torch.int64 else pc.random_keys(n, torch.int64, 0), begin, end).unique().shape[0] > 17


# ---- segments and ranges -------------------------------------------------------------------------------------------------

def test_segments_are_disjoint_out_of_order_and_leave_gaps():
  n, starts, ends = pc.segments_with_gaps()
  assert sorted(e - s for s, e in zip(starts, ends)) == sorted(pc.SEGMENT_LENGTHS)
  assert starts != sorted(starts)
  covered = np.zeros(n, dtype=np.int64)
  for s, e in zip(starts, ends):
    covered[s:e] += 1
  assert covered.max() == 1 and covered[0] == 0 and covered[-1] == 0 and (covered == 0).sum() >= 10
  k = torch.arange(n, 0, -1, dtype=torch.int32)
  v = torch.arange(n, dtype=torch.int32)
  ko, vo = pc.segmented_reference(k, v, starts, ends)
  outside = torch.from_numpy(covered == 0)
  assert torch.equal(ko[outside], k[outside]) and torch.equal(vo[outside], v[outside])
  s, e = starts[2], ends[2]
  assert torch.equal(ko[s:e], k[s:e].flip(0))


def test_ranges_reference():
  got = pc.ranges_reference([0, 0, 2, 2, 2, 5, 9, 9], 6)
  assert got.tolist() == [[0, 2], [0, 0], [2, 5], [0, 0], [0, 0], [5, 6]]
