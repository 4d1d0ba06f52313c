"""Shared inputs of the full-cloud evaluation tests (tests/test_eval_host.py, tests/test_gpu_eval.py): the nearest-neighbour cases
(i) to (viii) and a numpy restatement of the brute-force rule the grid search must reproduce bit for bit.

The rule: per query, over the processed points of its scene in ascending index, d = (dx * dx + dy * dy) + dz * dz with every
operation rounded to fp32; the best starts at 1e10 with the scene's first index and is replaced only by a STRICTLY smaller d — so
the answer is the lexicographic minimum of (d, index)."""
import functools

import numpy as np

DEFAULT_SIDE = 0.08      # 4 / voxel_scale at the shipped configs' 2 cm voxels


def brute_force_nn(xyz, ends, new_xyz, new_ends, chunk=1024):
    """-> (idx int32 [m], dist2 float32 [m]) by the rule above (numpy float32 arithmetic rounds every operation)."""
    xyz, new_xyz = np.asarray(xyz, np.float32), np.asarray(new_xyz, np.float32)
    idx = np.zeros(new_xyz.shape[0], np.int32)
    d2 = np.full(new_xyz.shape[0], np.float32(1e10), np.float32)
    s = qs = 0
    for e, qe in zip(ends, new_ends):
        p = xyz[s:e]
        idx[qs:qe] = s
        for q0 in range(qs, qe if e > s else qs, chunk):
            q = new_xyz[q0:min(qe, q0 + chunk)]
            dx, dy, dz = (q[:, None, k] - p[None, :, k] for k in range(3))
            d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == np.float32
            j = d.argmin(1)                       # the first minimum = the first strictly smaller candidate in ascending index
            best = d[np.arange(q.shape[0]), j]
            take = best < np.float32(1e10)
            idx[q0:q0 + q.shape[0]][take] = s + j[take]
            d2[q0:q0 + q.shape[0]][take] = best[take]
        s, qs = e, qe
    return idx, d2


def _ends(sizes):
    return np.cumsum(sizes).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (xyz float32 [n, 3], ends int32 [B], new_xyz float32 [m, 3], new_ends int32 [B], cell side in metres)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    f32 = np.float32
    if name in ("i", "vi_small", "vi_large"):
        # two scenes, sizes no multiple of 256, a workgroup of queries straddles the scene boundary; (vi): the same points with the
        # cell side forced to 1 mm (the 2^21-cell clamp doubles it) and to 100 m (a single cell)
        n, m = [3001, 2999], [11987, 12013]
        xyz = rng.uniform(0.0, 4.0, (sum(n), 3)).astype(f32)
        new = rng.uniform(0.0, 4.0, (sum(m), 3)).astype(f32)
        return xyz, _ends(n), new, _ends(m), {"i": DEFAULT_SIDE, "vi_small": 1e-3, "vi_large": 100.0}[name]
    if name == "ii":
        # a 0.25 m lattice with duplicate processed points, queries on the 0.125 m lattice: exact ties everywhere
        xyz = (rng.integers(0, 16, (3000, 3)) * 0.25).astype(f32)
        new = (rng.integers(0, 32, (8000, 3)) * 0.125).astype(f32)
        return xyz, _ends([3000]), new, _ends([8000]), DEFAULT_SIDE
    if name == "iii":
        # the full cloud from a box 1.5 x the processed one: queries outside the grid on every side
        xyz = rng.uniform(0.0, 4.0, (2000, 3)).astype(f32)
        new = rng.uniform(-1.0, 5.0, (8000, 3)).astype(f32)
        return xyz, _ends([2000]), new, _ends([8000]), DEFAULT_SIDE
    if name == "iv":
        # every processed point inside one cell but a single outlier 3 m away; queries around the outlier and between the two
        far = np.array([1.8, 1.7, 1.7], f32)
        xyz = np.concatenate((rng.uniform(0.0, 0.05, (500, 3)), far[None])).astype(f32)
        new = np.concatenate((far + rng.normal(0.0, 0.3, (300, 3)), rng.uniform(0.0, 1.0, (300, 1)) * far + rng.normal(0.0, 0.05, (300, 3))))
        return xyz, _ends([501]), new.astype(f32), _ends([600]), DEFAULT_SIDE
    if name == "v":
        return rng.uniform(0.0, 1.0, (1, 3)).astype(f32), _ends([1]), rng.uniform(-1.0, 2.0, (500, 3)).astype(f32), _ends([500]), DEFAULT_SIDE
    if name == "vii":
        # three scenes, the first with fewer processed points than a wave
        n, m = [37, 700, 900], [300, 2500, 3100]
        return (rng.uniform(0.0, 2.0, (sum(n), 3)).astype(f32), _ends(n), rng.uniform(-0.2, 2.2, (sum(m), 3)).astype(f32), _ends(m),
                DEFAULT_SIDE)
    if name == "viii":
        # a thin slab: z extent 0, a grid dimension of 1
        xyz = rng.uniform(0.0, 3.0, (2000, 3)).astype(f32)
        xyz[:, 2] = f32(0.5)
        new = rng.uniform(0.0, 3.0, (6000, 3)).astype(f32)
        new[:, 2] = rng.uniform(0.3, 0.7, 6000).astype(f32)
        return xyz, _ends([2000]), new, _ends([6000]), DEFAULT_SIDE
    raise KeyError(name)


CASES = ("i", "ii", "iii", "iv", "v", "vi_small", "vi_large", "vii", "viii")
