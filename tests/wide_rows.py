"""Arrays whose rows are wider than the 256 lanes of a row mover's workgroup (csrc/rows.h), for the densify and relocate
GPU tests: 256 / row_pieces is 0 there, every lane starts in row 0 and a row takes more than one round of the walk."""
import torch

N = 300                                            # one full block of 256 rows and a partial one
# floats per row -> pieces per row: 255 and 257 floats move as 4-byte pieces, 256 floats as 64 16-byte pieces,
# 1020 / 1024 / 1028 / 2052 floats as 255 / 256 / 257 / 513 16-byte pieces
WIDTHS = (255, 256, 257, 1020, 1024, 1028, 2052)
OFFSET_WIDTHS = (256, 1024)                        # on a base 4 bytes off a 16-byte boundary: 256 and 1024 4-byte pieces


def bits(t):
  return t.detach().contiguous().view(torch.int32)


def wide_arrays(device, seed=0):
  """{name: (N, width) float32 tensor on `device`} holding random BITS (NaN patterns included: compare with bits())."""
  g = torch.Generator().manual_seed(seed)
  words = lambda w: torch.randint(-2 ** 31, 2 ** 31 - 1, (N, w), dtype=torch.int32, generator=g).view(torch.float32)
  out = {}
  for w in WIDTHS:
    out[f'w{w}'] = words(w).to(device)
    assert out[f'w{w}'].data_ptr() % 16 == 0
  for w in OFFSET_WIDTHS:
    store = torch.zeros(N * w + 1, device=device)
    out[f'offset{w}'] = store[1:].view(N, w)
    out[f'offset{w}'].copy_(words(w))
    assert out[f'offset{w}'].data_ptr() % 16 == 4 and out[f'offset{w}'].is_contiguous()
  return out
