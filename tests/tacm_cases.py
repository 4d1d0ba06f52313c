"""The cases of tests/golden/tacm_golden.npz (made by tests/golden/make_tacm_golden.py from the reference's own tacm()), shared by
the maker and the tests: the inputs are regenerated from the seeds, the golden holds what the reference computed from them."""
import os

import numpy as np

N_CLASSES = 20
NUM_CLASS = 2                 # tail classes of the cuboid queue
FIX = float(1 << 28)          # include/doda_mix.h DODA_MIX_FIXED_BITS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tacm_golden.npz")

_BASE = dict(n_t=6000, n_s=5000, p=0.5, mix_ratio=0.5, permute_p=0.5, queue=True, queue_size=64, num_cuboid=2.0, tail=True, warm=True)
CASES = [
    dict(_BASE, seed=11, split=(2, 2, 1), p=1.0, permute_p=1.0, queue=False, tail=False),                  # mixed, permuted
    dict(_BASE, seed=12, split=(2, 1, 2), p=0.0, permute_p=0.0, queue=False, tail=False),                  # neither: the target, shrunk
    dict(_BASE, seed=13, split=(2, 2, 1), p=1.0, mix_ratio=1.0, permute_p=1.0, queue=False, tail=False),   # no target cuboid kept
    dict(_BASE, seed=14, split=(2, 2, 1), p=1.0, permute_p=0.0),                                           # queue, not permuted
    dict(_BASE, seed=15, split=(2, 1, 2), p=1.0, permute_p=1.0),                                           # queue, permuted
    dict(_BASE, seed=16, split=(2, 2, 1), p=0.0, permute_p=1.0, num_cuboid=2.5),                           # fractional num_cuboid
    dict(_BASE, seed=106, split=(3, 3, 2)),                                                                 # 18 cuboids
    dict(_BASE, seed=101, split=(2, 2, 1), warm=False),                                                     # queue enabled and empty
]


def scene(rng, n, tail):
    """fp32 [n, 3] points of a 6 x 5 x 3 m room somewhere near the origin and int64 labels: eight head classes everywhere, and —
    tail=True — 30 % of the points of the corner x, y < 2 m in classes 18 / 19 (uniformly random labels would put every tail
    class into every cuboid); 5 % ignored."""
    origin = rng.uniform(-1.0, 1.0, 3)
    rel = rng.random((n, 3)) * np.array([6.0, 5.0, 3.0])
    lab = rng.integers(0, 8 if tail else N_CLASSES, n)
    if tail:
        t = (rel[:, 0] < 2.0) & (rel[:, 1] < 2.0) & (rng.random(n) < 0.3)
        lab[t] = rng.choice(np.array([18, 19]), int(t.sum()))
    lab[rng.random(n) < 0.05] = 255
    return (rel + origin).astype(np.float32), lab.astype(np.int64)


def case_inputs(case):
    rng = np.random.default_rng(case["seed"])
    t_xyz, t_lab = scene(rng, case["n_t"], case["tail"])
    s_xyz, s_lab = scene(rng, case["n_s"], case["tail"])
    return t_xyz, t_lab, s_xyz, s_lab


def class_ratio_of(labels):
    """What pseudo_labels/class_ratio.txt would hold for these labels: the classes' shares of the labelled points."""
    lab = labels[(labels >= 0) & (labels < N_CLASSES)]
    h = np.bincount(lab, minlength=N_CLASSES).astype(np.float64)
    return h / h.sum()


# SplitSampler / Queue against the reference's classes
SAMPLER_CLASS_RATIO = np.array([0.31, 0.22, 0.0, 0.09, 0.004, 0.07, 0.05, 0.0, 0.011, 0.03, 0.02, 0.06, 0.002, 0.04, 0.03, 0.02,
                                0.018, 0.015, 0.006, 0.004])
SAMPLER_SIZE = 64
QUEUE_UPDATES = [[1, 2, 3], [4], [5, 6, 7], [], [8, 9, 10, 11, 12, 13, 14], [15, 16]]      # a ring of 5: wraps, and truncates 7 to 5
SAMPLER_RATIO_STEPS = [[3.0, 0.0, 1.0], [0.0, 0.0, 0.0], [10.0, 250.0, 40.0]]


def load_case(z, i):
    """Case i of the opened golden -> dict (draws as the [(kind, value)] list ReplayDraws takes)."""
    pre = "c%d_" % i
    d = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    draws, at = [], 0
    for kind, n in zip(d["draw_kinds"], d["draw_lens"]):
        if n < 0:
            draws.append((str(kind), float(d["draw_vals"][at])))
            at += 1
        else:
            draws.append((str(kind), d["draw_vals"][at:at + n].copy()))
            at += n
    d["draws"] = draws
    d["items"] = [d["item%d" % q] for q in range(int(d["n_items"]))]
    return d
