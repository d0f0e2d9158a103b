"""The pixel rows a render stores, and the addresses its kernels get for them.

A frame may render a window of tile rows only (the strips of ``distributed.py`` / ``sharded.py``), and a CROPPED render
allocates nothing but that window's pixel rows [y0, y1).  The kernels address absolute rows, so a tensor laid out in the
window is handed to them as the address its row 0 WOULD have; they touch rows [y0, y1) only.  ``RowWindow.base`` is the one
place in the package that forms such an address, and the one place that deals with the window that stores no row at all:
a zero-row tensor has a null data pointer, which the C entry points reject and from which an offset would wrap."""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch


class RowWindow(NamedTuple):
  """Build with ``RowWindow.of``."""
  w: int
  h: int
  rows: Tuple[int, int]     # tile rows, clamped as frame_geom (csrc/frame.hip) clamps them; end <= begin: nothing is rendered
  y0: int                   # the pixel rows [y0, y1) of those tile rows
  y1: int
  cropped: bool             # output tensors hold rows [y0, y1) only, not all h
  whole: bool               # the tile rows are the whole frame

  @classmethod
  def of(cls, image_size, tile_size: int, tile_rows=None, cropped: bool = False) -> 'RowWindow':
    w, h = int(image_size[0]), int(image_size[1])
    tiles_high = (h + tile_size - 1) // tile_size
    rows = (0, tiles_high) if tile_rows is None else (max(0, int(tile_rows[0])), min(tiles_high, int(tile_rows[1])))
    return cls(w, h, rows, min(rows[0] * tile_size, h), min(rows[1] * tile_size, h), bool(cropped), rows == (0, tiles_high))

  @property
  def px_rows(self) -> Tuple[int, int]:
    return self.y0, self.y1

  @property
  def stored_rows(self) -> int:
    return max(self.y1 - self.y0, 0) if self.cropped else self.h

  @property
  def zero_filled(self) -> bool:
    """rows outside the window exist in the output and are not rendered"""
    return not self.cropped and not self.whole

  def alloc(self, dtype, device, channels: Optional[int] = None, scratch: bool = False) -> torch.Tensor:
    """An output laid out in the window: (rows, w, channels), or (rows, w) without ``channels``.  ``scratch``: nobody
    reads it outside the window's rows, so it is never filled."""
    shape = (self.stored_rows, self.w) if channels is None else (self.stored_rows, self.w, channels)
    return (torch.zeros if self.zero_filled and not scratch else torch.empty)(shape, dtype=dtype, device=device)

  def placeholder(self, dtype, device) -> Optional[torch.Tensor]:
    """None — or, for a window that stores no row, the tensor whose address ``base`` hands out instead: the kernels
    touch no row, any valid address will do.  Whoever passes the addresses on keeps it alive as long as they are used."""
    return torch.empty((16,), dtype=dtype, device=device) if self.stored_rows == 0 else None

  def base(self, tensor: torch.Tensor, channels: int = 1, placeholder: Optional[torch.Tensor] = None) -> int:
    """The address to hand a kernel for ``tensor`` (contiguous, ``stored_rows`` rows of w x channels elements)."""
    assert tensor.shape[0] == self.stored_rows, f"a tensor of {tensor.shape[0]} rows in a window of {self.stored_rows}"
    if self.stored_rows == 0:
      assert placeholder is not None, "a window that stores no row: pass its placeholder()"
      return placeholder.data_ptr()
    return tensor.data_ptr() - (self.y0 if self.cropped else 0) * self.w * channels * tensor.element_size()
