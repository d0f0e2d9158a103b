"""csrc/rows.h without a GPU: the division-free (row, piece in row) walk of the row movers against divmod, compiled for
the host from the header itself, and the descriptor checks that ms_densify_move and ms_relocate_move share."""
import ctypes
import subprocess
from pathlib import Path

import pytest

from taichi_splatting_amd import _lib

CSRC = Path(__file__).resolve().parent.parent / 'taichi_splatting_amd' / 'csrc'

WALK = r"""
#include <stdio.h>
#include "rows.h"

// PieceWalk(lane, row_pieces) followed for row_pieces advances: (r, k) == divmod(lane + 256 step, row_pieces) at every step
static long follow(uint32_t row_pieces, uint32_t lane) {
  ms::PieceWalk w(lane, row_pieces);
  for (uint32_t step = 0; step <= row_pieces; ++step) {
    const uint64_t p = (uint64_t)lane + (uint64_t)ms::ROW_BLOCK * step;
    if (w.r != p / row_pieces || w.k != p % row_pieces) {
      printf("row_pieces %u lane %u step %u: walk (%u, %u), divmod (%llu, %llu)\n", row_pieces, lane, step, w.r, w.k,
             (unsigned long long)(p / row_pieces), (unsigned long long)(p % row_pieces));
      return -1;
    }
    w.advance();
  }
  return (long)row_pieces + 1;
}

int main() {
  static_assert(ms::ROW_BLOCK == 256 && ms::ROW_UNROLL == 4 && ms::ROW_MAX_ARRAYS == 32, "constants of rows.h");
  static_assert(ms::ROW_MAX_BYTES == (1 << 20) && ms::ROW_FLAG_BIT == (1 << 30), "constants of rows.h");
  long checked = 0;
  for (uint32_t row_pieces = 1; row_pieces <= 1100; ++row_pieces)
    for (uint32_t lane = 0; lane < 256; ++lane) {
      const long n = follow(row_pieces, lane);
      if (n < 0) return 1;
      checked += n;
    }
  const uint32_t wide[3] = {4096, 65536, 262144}, lanes[3] = {0, 1, 255};
  for (uint32_t row_pieces : wide)
    for (uint32_t lane : lanes) {
      const long n = follow(row_pieces, lane);
      if (n < 0) return 1;
      checked += n;
    }
  printf("ok %ld\n", checked);
  return 0;
}
"""


def test_piece_walk_is_divmod(tmp_path):
  """Every row width up to 1100 pieces from every lane (both sides of 256 pieces, where 256 / row_pieces becomes 0 and
  every lane starts in row 0), and the widest rows the entry points accept (1 MiB: 65536 and 262144 pieces)."""
  src, exe = tmp_path / 'walk.cpp', tmp_path / 'walk'
  src.write_text(WALK)
  subprocess.run(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-I', str(CSRC), str(src), '-o', str(exe)], check=True)
  run = subprocess.run([str(exe)], capture_output=True, text=True)
  assert run.returncode == 0, run.stdout
  steps = 256 * sum(w + 1 for w in range(1, 1101)) + 3 * sum(w + 1 for w in (4096, 65536, 262144))
  assert run.stdout.split() == ['ok', str(steps)]


# ---- check_row_array through its two callers: null or dummy pointers, n > 0, so a pass would reach a launch ------------

def descriptors(cls, base_field, good, second=False, base=None, **bad):
  """One descriptor with the fields of `bad` (base: the address of its main array), behind a good one if `second`."""
  if base is not None:
    bad[base_field] = base
  wrong = cls(**{**good, **bad})
  return (cls * 2)(cls(**good), wrong) if second else (cls * 1)(wrong)


def densify_move(lib, **kw):
  good = dict(struct_size=ctypes.sizeof(_lib.DensifyArrayC), child_fill=1, src=256, dst=512, row_bytes=16)
  arrays = descriptors(_lib.DensifyArrayC, 'src', good, **kw)
  return lib.ms_densify_move(arrays, len(arrays), 256, 256, 10, 10, None)


def relocate_move(lib, **kw):
  good = dict(struct_size=ctypes.sizeof(_lib.RelocateArrayC), role=_lib.RELOCATE_COPY, data=256, fresh=None, row_bytes=16)
  arrays = descriptors(_lib.RelocateArrayC, 'data', good, **kw)
  return lib.ms_relocate_move(arrays, len(arrays), 256, 256, 10, None)


CASES = [
  ('struct_size', dict(struct_size=16), -4),
  ('row_bytes 0', dict(row_bytes=0), -1),
  ('row_bytes -4', dict(row_bytes=-4), -1),
  ('row_bytes 6', dict(row_bytes=6), -1),
  ('row_bytes 1 MiB + 4', dict(row_bytes=(1 << 20) + 4), -1),
  ('base at address 2', dict(base=2), -1),
  ('second descriptor bad', dict(second=True, row_bytes=6), -1),
  ('second descriptor of another ABI', dict(second=True, struct_size=16), -4),
]


@pytest.mark.parametrize('name,kw,code', CASES, ids=[c[0] for c in CASES])
def test_both_movers_check_a_descriptor_alike(lib, name, kw, code):
  err = lambda: lib.ms_last_error_string().decode()
  assert densify_move(lib, **kw) == code
  densify_text = err()
  assert relocate_move(lib, **kw) == code
  relocate_text = err()
  assert densify_text.startswith('ms_densify_move: ') and relocate_text.startswith('ms_relocate_move: ')
  assert densify_text.replace('ms_densify_', 'ms_X_') == relocate_text.replace('ms_relocate_', 'ms_X_')
  if 'second' in kw and code == -1:
    assert 'array 1' in densify_text


def test_descriptor_messages_are_the_documented_ones(lib):
  """The texts a caller may have matched on, byte for byte."""
  err = lambda: lib.ms_last_error_string().decode()
  size = ctypes.sizeof(_lib.DensifyArrayC)
  assert densify_move(lib, struct_size=16) == -4
  assert err() == f"ms_densify_move: ms_densify_array of another ABI (struct_size 16, this library: {size})"
  assert relocate_move(lib, struct_size=16) == -4
  assert err() == f"ms_relocate_move: ms_relocate_array of another ABI (struct_size 16, this library: {ctypes.sizeof(_lib.RelocateArrayC)})"
  assert relocate_move(lib, second=True, row_bytes=(1 << 20) + 4) == -1
  assert err() == "ms_relocate_move: array 1: row_bytes must be a positive multiple of 4, at most 1048576 (got 1048580)"
  assert densify_move(lib, row_bytes=-4) == -1
  assert err() == "ms_densify_move: array 0: row_bytes must be a positive multiple of 4, at most 1048576 (got -4)"
  assert densify_move(lib, base=2) == -1
  assert err() == "ms_densify_move: array 0: bases must be 4-byte aligned"
  assert relocate_move(lib, base=2) == -1
  assert err() == "ms_relocate_move: array 0: bases must be 4-byte aligned"
