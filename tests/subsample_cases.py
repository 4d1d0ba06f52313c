"""The training subsample (include/doda_subsample.h) restated in numpy: the key function of doda_amd/csrc/subsample_key.hpp in
uint32 / uint64 arithmetic, the selection by a plain np.lexsort, and the cases both the host and the GPU tests run."""
import numpy as np

M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
LOW = np.uint64(0xffffffff)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays, key: two ints -> the four output words (Random123's Philox-4x32-10)."""
    c = [np.asarray(v, dtype=np.uint64) for v in counter]
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                    # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & LOW, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & LOW]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return [v.astype(np.uint32) for v in c]


def keys(seed, n, key_mask=0xffffffff):
    """uint32 [n]: key(seed, j) & key_mask for j = 0 .. n - 1."""
    j = np.arange(n, dtype=np.uint64)
    z = np.zeros(n, dtype=np.uint64)
    seed = int(seed) & 0xffffffffffffffff
    return philox4x32_10((j, z, z, z), (seed & 0xffffffff, seed >> 32))[0] & np.uint32(key_mask)


def select(seed, n, k, key_mask=0xffffffff):
    """int64 [k]: the k points smallest in the lexicographic order (key, index), in ascending index."""
    order = np.lexsort((np.arange(n), keys(seed, n, key_mask)))     # (the last key is the primary one)
    return np.sort(order[:k])


def count(n, ds):
    return int(n / ds)


def scene(n, seed):
    """(xyz float32 [n, 3] with every bit pattern class that a copy must keep — negative zero, a NaN payload, a denormal — and labels)."""
    rng = np.random.default_rng(seed)
    xyz = rng.standard_normal((n, 3)).astype(np.float32)
    if n >= 3:
        xyz[0, 0], xyz[1, 1] = -0.0, np.float32(1e-42)
        xyz.view(np.uint32)[2, 2] = 0x7fc12345
    return xyz, rng.integers(0, 20, n).astype(np.int32)


def case(sizes, ks, seed0=1234, key_mask=0xffffffff):
    return {"sizes": list(sizes), "ks": list(ks), "seeds": [(seed0 * 0x9E3779B97F4A7C15 + 77 * b) & 0xffffffffffffffff for b in range(len(sizes))],
            "key_mask": key_mask}


def cases():
    out = {}
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000):      # wave and chunk edges
        for ds in (1, 3, 4):
            out["n%d_ds%d" % (n, ds)] = case([n], [count(n, ds)], seed0=n * 10 + ds)
    out["k1"] = case([5000], [1])
    out["k_n_minus_1"] = case([5000], [4999])
    out["four_segments"] = case([5000, 1, 0, 3333], [1250, 1, 0, 833])
    out["32_segments"] = case([100] * 32, [25] * 32)
    for mask in (0xF, 0x1, 0x0):
        out["ties_mask_%x" % mask] = case([5000], [1250], key_mask=mask)
    out["ties_two_segments"] = case([2049, 2049], [700, 700], key_mask=0x3)
    return out


def inputs(c):
    """(xyz [N, 3], labels [N], offsets) of a case."""
    parts = [scene(n, 1000 + b) for b, n in enumerate(c["sizes"])]
    offsets = np.concatenate(([0], np.cumsum(c["sizes"]))).astype(np.int64)
    return (np.concatenate([p[0] for p in parts]).reshape(-1, 3), np.concatenate([p[1] for p in parts]).astype(np.int32),
            [int(v) for v in offsets])


def expected(c):
    """(sub_idx int32 [K], rows int64 [K] into the concatenation, offsets_s) by the restatement."""
    subs, rows, offsets_s, at = [], [], [0], 0
    for n, k, seed in zip(c["sizes"], c["ks"], c["seeds"]):
        sub = select(seed, n, k, c["key_mask"])
        subs.append(sub)
        rows.append(sub + at)
        offsets_s.append(offsets_s[-1] + k)
        at += n
    return np.concatenate(subs).astype(np.int32), np.concatenate(rows).astype(np.int64), offsets_s
