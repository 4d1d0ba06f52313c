"""Host side of the segment layer (csrc/segments.hpp) that doda_amd.tacm and doda_amd.aug share: a batch is segments of one array,
its B + 1 host offsets travel with every native call, the launches go to one stream, and every random number of a sample comes from
one `draws` object."""
import contextlib
import ctypes as C

import numpy as np
import torch

from . import _lib


def offsets_h(offsets):
    """B + 1 host integers -> (c_int64 array, n_seg) as the native calls take them."""
    arr = (C.c_int64 * len(offsets))(*[int(v) for v in offsets])
    return arr, len(offsets) - 1


def stream_handle(stream):
    """The raw handle of `stream` (a torch stream or a handle); None: torch's current stream."""
    if stream is not None:
        return stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
    from .ops import _stream as cur
    return cur()


@contextlib.contextmanager
def launch_on(stream):
    """torch's own launches (allocations' stream, copies, read-backs) on `stream` too, where it is a torch stream."""
    if stream is not None and hasattr(stream, "cuda_stream"):
        with torch.cuda.stream(stream):
            yield
    else:
        yield


def n_blocks(L, symbol, offsets):
    """Workgroups (chunks) of a batch: L.<symbol>(offsets), one of doda_mix_blocks / doda_aug_blocks."""
    arr, n_seg = offsets_h(offsets)
    nb = getattr(L, symbol)(arr, n_seg)
    if nb < 0:
        raise _lib.DodaNativeError("%s: invalid segment offsets" % symbol)
    return int(nb)


def per_sample(draws, n, who):
    """One draws object per sample as a list (one object alone stands for a batch of one)."""
    if not isinstance(draws, (list, tuple)):
        draws = [draws]
    if len(draws) != n:
        raise ValueError("%s: one draws object per sample" % who)
    return draws


class SeededDraws:
    """The production `draws` object: every random number of a sample from one seeded numpy generator."""

    def __init__(self, seed):
        self.g = np.random.default_rng(seed)

    def rand(self, n=None):
        return self.g.random() if n is None else self.g.random(n)

    def randn(self, shape):
        return self.g.standard_normal(tuple(int(v) for v in shape))

    def randint(self, n):
        return int(self.g.integers(int(n)))

    def permutation(self, n):
        return self.g.permutation(n)

    def choice(self, n, k, p):
        return self.g.choice(n, k, p=np.asarray(p, dtype=np.float64) / np.sum(p))

    def sample(self, k, n):
        return [int(v) for v in self.g.choice(n, k, replace=False)]
