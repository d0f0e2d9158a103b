"""Host-side machinery of the frame executor that does not depend on the frame logic (``frame.py`` re-exports it): the
pinned words the frames' K kernels write, the persistent accumulators of the raster backward, the parked collector."""
from __future__ import annotations

import collections
import contextlib
import gc
import threading
import time
import weakref

import torch

from . import _lib

_lock = threading.RLock() # guards the executor's caches and serialises the enqueue of a backward pass (ctypes drops the GIL)
_k_host = {}              # device index -> KSlots: a ring of pinned int32 words, ONE PER FRAME IN FLIGHT
_moments = collections.OrderedDict()   # (device index, stream, n, deterministic) -> accumulator rows, zero between frames
_moments_pinned = set()   # keys whose buffer address is baked into a captured HIP graph: never evicted

MOMENTS_LRU = 4           # accumulator buffers kept per device (scene sizes / streams alternating in one process)
K_SLOTS = 64              # pinned K words per device; a frame holds one from its forward until it has looked at K
GRAPH_K_WORDS = 1024      # pinned K words per device for frames captured into HIP graphs
K_PENDING = -(1 << 31)      # sentinel the host writes into the pinned word before a frame; K itself is >= 0


def pinned_word():
  """(pinned int32[1] tensor, its numpy view)"""
  word = torch.zeros((1,), dtype=torch.int32).pin_memory()
  return word, word.numpy()


class KSlots:
  """Pinned int32 words the frames' K kernels write (``ms_frame_project_count(k_host)``), one per frame in flight.

  Round 3 kept ONE word per device: a second frame enqueued before the first had looked at its overlap total (a
  viewer thread next to a training thread, two frames rendered back to back before either is settled) reset the
  word and the first frame then validated its capacity against the other frame's K."""

  def __init__(self):
    self.words = torch.zeros((K_SLOTS,), dtype=torch.int32).pin_memory()
    self.view = self.words.numpy()
    self.busy = [False] * K_SLOTS
    self.next = 0
    # words for frames captured into HIP graphs (kept for the life of the process: a graph replays into its word).
    # Allocated HERE, in eager mode: pinning host memory inside a stream capture invalidates the capture
    # (hipHostMalloc is not a capturable call — seen at 6 M gaussians, where torch's host cache had no block to reuse)
    self.graph_words = torch.zeros((GRAPH_K_WORDS,), dtype=torch.int32).pin_memory()
    self.graph_view = self.graph_words.numpy()
    self.graph_next = 0
    self.graph_free = []

  def acquire_for_graph(self, state):
    """a word for a frame being captured; it returns to the pool when the frame's state (kept alive by the graph's
    result) is garbage collected"""
    with _lock:
      if self.graph_free:
        i = self.graph_free.pop()
      else:
        i = self.graph_next
        if i >= GRAPH_K_WORDS:
          raise RuntimeError(f"more than {GRAPH_K_WORDS} live frames captured into HIP graphs in this process")
        self.graph_next = i + 1
    weakref.finalize(state, self.graph_free.append, i)
    return self.graph_words[i:i + 1], self.graph_view[i:i + 1]

  def acquire(self):
    """(slot index or -1, one-element pinned tensor, its numpy view)"""
    with _lock:
      for _ in range(K_SLOTS):
        i = self.next
        self.next = (i + 1) % K_SLOTS
        if not self.busy[i]:
          self.busy[i] = True
          return i, self.words[i:i + 1], self.view[i:i + 1]
    return (-1, *pinned_word())          # more than K_SLOTS unsettled frames: a private word

  def release(self, i):
    if i >= 0:
      self.busy[i] = False


def k_ring(device) -> KSlots:
  with _lock:
    ring = _k_host.get(device.index)
    if ring is None:
      ring = _k_host[device.index] = KSlots()
  return ring


def wait_for_k(k_np, k_event):
  """The host's one wait per eager frame: (overlap total, whether it had to wait).  Polling the pinned word the K kernel
  writes returns within microseconds of the write; ``Event.synchronize`` (an interrupt-driven sleep) cost 0.3-0.5 ms of
  wake-up latency per frame, which at 1 M gaussians left the GPU idle for a third of the frame."""
  deadline = time.perf_counter() + 2.0
  spins = 0
  while k_np[0] == K_PENDING:
    spins += 1
    if spins & 63 == 0:
      time.sleep(0)                         # let other Python threads run: the poll holds the GIL otherwise
      if time.perf_counter() > deadline:    # never seen; a lost write must not hang the caller
        k_event.synchronize()
        break
  return int(k_np[0]), spins > 0


@contextlib.contextmanager
def parked_gc():
  """Run a training / timing loop with Python's cyclic collector parked.

  An eager frame keeps the GPU about one frame ahead of the host (the one wait per frame is for the overlap total).
  A generation-2 collection walks every tracked object of the process — with torch imported, 35-45 ms, i.e. ten
  config-D frames — about once every couple of hundred frames, and the GPU idles for most of it
  (``tools/host_overhead.py``: frame intervals median 3.40 ms, max 44 ms; 11 ms with the collector parked).
  Reference counting still frees every tensor of a frame when the frame ends; only cycle detection is deferred to
  the end of the block.  (A HIP-graph replay, ``FrameGraph``, needs no host per frame and is not affected.)"""
  was_enabled = gc.isenabled()
  gc.collect()
  gc.freeze()
  gc.disable()
  try:
    yield
  finally:
    gc.unfreeze()
    if was_enabled:
      gc.enable()


def release_moments(force: bool):
  """Accumulators whose address a captured HIP graph replays into (``FrameGraph`` / ``torch.cuda.graph``) are kept unless
  ``force`` — freeing them would let the next replay accumulate into memory the allocator has handed to someone else."""
  with _lock:
    for key in list(_moments):
      if force or key not in _moments_pinned:
        del _moments[key]
    if force:
      _moments_pinned.clear()


def _moments_buffer(device, n: int, deterministic: bool) -> torch.Tensor:
  """Persistent (n, MOMENT_ROW) accumulator of the raster backward: zero on entry of every backward pass, and zero
  again when it returns (the per-gaussian pass clears the rows it reads) — no 64 B-per-gaussian fill per frame.

  One buffer per (device, stream, size, mode): two backward passes on DIFFERENT streams never share rows (on one
  stream they run one after the other and the rows are zero in between).  A small LRU per device instead of "one
  size at a time": alternating two scene sizes (a 3D model and ``rasterize()`` of a 2D set) no longer reallocates and
  zero-fills on every backward.  A buffer handed out during HIP-graph capture is pinned: its address is part of the
  graph."""
  stream = int(torch.cuda.current_stream(device).cuda_stream)
  key = (device.index, stream, int(n), bool(deterministic))
  with _lock:
    buf = _moments.get(key)
    if buf is None and torch.cuda.is_current_stream_capturing():
      # a capture runs on a stream of its own: take the accumulator the eager warm-up frames of this scene size used
      # (zero between frames) instead of allocating AND ZERO-FILLING a new one inside the graph — the fill would be
      # replayed with every step (384 MB at 6 M gaussians)
      for other, cand in _moments.items():
        if (other[0], other[2], other[3]) == (key[0], key[2], key[3]):
          buf = _moments[key] = cand
          _moments_pinned.add(other)
          break
    if buf is None:
      mine = [k for k in _moments if k[0] == device.index and k not in _moments_pinned]
      for k in mine[:max(0, len(mine) - (MOMENTS_LRU - 1))]:
        del _moments[k]                     # least recently used first (OrderedDict order)
      buf = _moments[key] = torch.zeros((max(n, 1), _lib.MOMENT_ROW),
                                        dtype=torch.int64 if deterministic else torch.float32, device=device)
    else:
      _moments.move_to_end(key)
    if torch.cuda.is_current_stream_capturing():
      _moments_pinned.add(key)
  return buf


def _drop_moments():
  """After a failed backward enqueue the accumulator rows may be half-written: start from clean ones.  Buffers whose
  address a captured HIP graph replays into are zeroed IN PLACE (freeing them would let the next replay accumulate into
  memory the allocator has handed to someone else — what ``release_caches`` guards against with ``force``); the others
  are dropped and reallocated on demand."""
  with _lock:
    for key in list(_moments):
      if key not in _moments_pinned:
        del _moments[key]
        continue
      buf = _moments[key]
      if torch.cuda.is_current_stream_capturing():
        continue              # (a failure inside a capture: the capture is lost anyway, and a fill must not join it)
      # on the buffer's OWN stream (key[1]): the graph that replays into it runs there, and a fill on whatever stream
      # is current could race with a replay in flight
      own = torch.cuda.ExternalStream(key[1], device=buf.device) if key[1] else torch.cuda.default_stream(buf.device)
      with torch.cuda.stream(own):
        buf.zero_()
