"""Seeded inputs of the Lovasz-softmax tests (tests/golden/make_lovasz_golden.py, test_lovasz_host.py, test_gpu_lovasz.py):
regenerated from the seeds, not stored.

A case is a voxel-level head problem: features [m, 16], head weights [n_cls, 16] and bias [n_cls], the voxel -> point lists and the
point labels.  Features, weights and bias are drawn from dyadic grids (k / 64 and k / 128, at most 8 significant bits), so that
  * they are exact in bf16 as well as fp32: the bf16 and the fp32 device runs and the host see the same numbers, and
  * every product and partial sum of W f + b is exact in fp32: the case's logits `z` (fp64, from these inputs) are the logits the
    device computes, and the comparison isolates what the loss itself adds (softmax, sort, Jaccard differences).
The first five are the shapes of the issue's table (voxels, classes, valid points, absent classes, ignored share); 6: the logits
of case 1 times 40 (probabilities saturate: ties at errors 0 and 1; the logits keep a grid of 5 / 1024, fine enough that
unsaturated probabilities of different voxels do not tie, which would leave the gradient to the sort's tie order); 7: 5000 voxels with 1-3 points each (about 110 k items:
several tiles of every kernel per class); 8: 4097 voxels, 32 classes."""
import numpy as np

IGNORE = 255
C = 16

#        m   n_cls valid absent ignored scale  points per voxel
SPECS = [
    dict(m=300, n_cls=11, valid=760, absent=1, ignored=0.20),
    dict(m=1, n_cls=2, valid=5, absent=0, ignored=0.0),
    dict(m=700, n_cls=13, valid=1425, absent=2, ignored=0.50),
    dict(m=257, n_cls=8, valid=257, absent=0, ignored=0.10),
    dict(m=64, n_cls=20, valid=220, absent=3, ignored=0.30),
    dict(m=300, n_cls=11, valid=760, absent=1, ignored=0.20, scale=40, seed=0),      # case 1's inputs, logits x 40
    dict(m=5000, n_cls=11, per_voxel=(1, 3), absent=0, ignored=0.20),
    dict(m=4097, n_cls=32, per_voxel=(1, 2), absent=0, ignored=0.10),
]
N_CASES = len(SPECS)


def make_case(i):
    """-> dict(feats [m,16], weight [n_cls,16], bias [n_cls] (float64, exact in bf16), z [m,n_cls] float64 = feats W^T + b,
    v2p int32 [m, 1 + max points], p2v int64 [points], labels int64 [points], n_cls, m)."""
    s = SPECS[i]
    rng = np.random.RandomState(1000 + s.get("seed", i))
    m, n_cls, scale = s["m"], s["n_cls"], s.get("scale", 1)
    feats = rng.randint(-127, 128, (m, C)).astype(np.float64) / 64                   # 7 bits
    weight = rng.randint(-48, 49, (n_cls, C)).astype(np.float64) / 128 * scale       # 6 bits; x 40 = 5 k / 16: 8 bits
    bias = rng.randint(-48, 49, (n_cls,)).astype(np.float64) / 128 * scale
    z = feats @ weight.T + bias
    if "per_voxel" in s:
        counts = rng.randint(s["per_voxel"][0], s["per_voxel"][1] + 1, m)
        n_points = int(counts.sum())
        n_ignored = int(round(s["ignored"] * n_points))
    else:
        n_points = int(round(s["valid"] / (1.0 - s["ignored"])))
        n_ignored = n_points - s["valid"]
        counts = np.ones(m, dtype=np.int64) + np.bincount(rng.randint(0, m, n_points - m), minlength=m)
    p2v = rng.permutation(np.repeat(np.arange(m), counts))
    v2p = np.zeros((m, 1 + int(counts.max())), dtype=np.int32)
    for p in np.argsort(p2v, kind="stable"):
        v = p2v[p]
        v2p[v, 0] += 1
        v2p[v, v2p[v, 0]] = p
    present = np.sort(rng.permutation(n_cls)[s["absent"]:])
    labels = present[rng.randint(0, len(present), n_points)].astype(np.int64)
    ignored = rng.permutation(n_points)[:n_ignored]
    labels[ignored] = IGNORE
    kept = np.flatnonzero(labels != IGNORE)
    labels[kept[:len(present)]] = present                   # every class that is not absent occurs among the valid points
    return dict(feats=feats, weight=weight, bias=bias, z=z, v2p=v2p, p2v=p2v.astype(np.int64), labels=labels, n_cls=n_cls, m=m,
                n_valid=int((labels != IGNORE).sum()), absent=s["absent"])
