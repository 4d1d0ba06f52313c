"""Numpy restatements of the clustering, segment-pool and proposal-IoU operators of include/doda_pgops.h, written from their
semantics (the reference's PG_OP: a sequential BFS over ball-query lists; per-segment mean / min / max / arg-max with strict
compares; intersection over union from counts), and the designed inputs the host and GPU tests share.

Conventions restated here as the ABI states them: a list or segment range is clamped to its array, end < start is empty, a
neighbour or point index outside [0, N) is skipped."""
import numpy as np

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------------------------------------------------------
class Graph:
    def __init__(self, name, label, idxs, start_len, symmetric):
        self.name, self.symmetric = name, symmetric
        self.label = np.asarray(label, dtype=np.int32)
        self.idxs = np.asarray(idxs, dtype=np.int32)
        self.start_len = np.asarray(start_len, dtype=np.int32).reshape(-1, 2)
        self.n = self.label.shape[0]

    def neighbours(self, i):
        """The valid entries of i's list, in list order."""
        na = self.idxs.shape[0]
        st, ln = int(self.start_len[i, 0]), int(self.start_len[i, 1])
        lo = min(max(st, 0), na)
        hi = max(min(st + ln, na), lo)
        js = self.idxs[lo:hi]
        return js[(js >= 0) & (js < self.n)]


def pack(name, label, lists, symmetric):
    idxs, start_len, pos = [], [], 0
    for l in lists:
        start_len.append((pos, len(l)))
        idxs.extend(int(j) for j in l)
        pos += len(l)
    return Graph(name, label, np.asarray(idxs, dtype=np.int64).astype(np.int32), start_len, symmetric)


def _symmetrise(lists):
    sets = [set(l) for l in lists]
    for i, l in enumerate(lists):
        for j in l:
            if i not in sets[j]:
                sets[j].add(i)
                lists[j].append(i)
    return lists


def random_graph(n, seed, symmetric=True, n_labels=3, degree=2, window=9):
    """Sparse random lists among near indices (several components of several sizes), labels in runs."""
    rng = np.random.default_rng(seed)
    label = (np.arange(n) // 7 + rng.integers(0, 2, n)) % n_labels
    lists = [[] for _ in range(n)]
    for i in range(n):
        for _ in range(int(rng.integers(0, degree + 1))):
            j = int(np.clip(i + rng.integers(-window, window + 1), 0, n - 1))
            lists[i].append(j)
    if symmetric:
        _symmetrise(lists)
    return pack("random%d" % n, label, lists, symmetric)


def chain(n=4096):
    lists = [[j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)]
    return pack("chain", np.zeros(n), lists, True)


def star(spokes=5000, hub=2500):
    n = spokes + 1
    lists = [[hub] for _ in range(n)]
    lists[hub] = [j for j in range(n) if j != hub]
    return pack("star", np.zeros(n), lists, True)


def grid(side=40, patch=8):
    """4-connected side x side grid; labels alternate in a checkerboard of patch x patch squares, so every patch is a component."""
    n = side * side
    y, x = np.divmod(np.arange(n), side)
    label = ((y // patch) + (x // patch)) % 2
    lists = []
    for i in range(n):
        l = []
        if y[i] > 0: l.append(i - side)
        if x[i] > 0: l.append(i - 1)
        if x[i] < side - 1: l.append(i + 1)
        if y[i] < side - 1: l.append(i + side)
        lists.append(l)
    return pack("grid", label, lists, True)


def empty_lists(n=100):
    return pack("empty", np.arange(n) % 2, [[] for _ in range(n)], True)


def self_and_duplicates(n=300, seed=5):
    g = random_graph(n, seed)
    lists = [list(g.neighbours(i)) for i in range(n)]
    for i in range(0, n, 3):
        lists[i] = [i] + lists[i] + lists[i][:2] + [i]
    return pack("selfdup", g.label, lists, True)


def out_of_range(n=300, seed=6):
    g = random_graph(n, seed)
    junk = [-1, n, n + 5, -2 ** 31, 2 ** 31 - 1]
    lists = [list(g.neighbours(i)) for i in range(n)]
    for i in range(0, n, 4):
        lists[i] = [junk[i % 5]] + lists[i] + [junk[(i + 1) % 5]]
    return pack("outofrange", g.label, lists, True)


def asymmetric(n=400, seed=7):
    return random_graph(n, seed, symmetric=False)


def corrupt_ranges(n=200, seed=8):
    """start / len pairs that leave the array: negative starts, negative lengths, ends past nActive."""
    g = random_graph(n, seed, symmetric=False)
    sl = g.start_len.copy()
    na = g.idxs.shape[0]
    sl[3] = (-4, 9)
    sl[10] = (5, -2)
    sl[17] = (na - 2, 50)
    sl[30] = (na + 10, 3)
    sl[41] = (2 ** 31 - 1, 2 ** 31 - 1)
    sl[55] = (-2 ** 31, 2 ** 31 - 1)
    return Graph("corrupt_ranges", g.label, g.idxs, sl, False)


SIZES = (0, 1, 2, 63, 64, 65, 1025)


def graph_cases():
    cases = [random_graph(n, 100 + n) for n in SIZES]
    cases += [chain(), star(), grid(), empty_lists(), self_and_duplicates(), out_of_range(), asymmetric(), corrupt_ranges()]
    return cases


def bfs_clusters(g, threshold):
    """The sequential rule: seeds ascending, a queue, directed edges, a first-visit mark.  -> list of point lists."""
    visited = np.zeros(g.n, dtype=bool)
    out = []
    for seed in range(g.n):
        if visited[seed]:
            continue
        comp, head = [seed], 0
        visited[seed] = True
        while head < len(comp):
            cur = comp[head]
            head += 1
            for j in g.neighbours(cur):
                if g.label[j] == g.label[cur] and not visited[j]:
                    visited[j] = True
                    comp.append(int(j))
        if len(comp) >= threshold:
            out.append(comp)
    return out


def components(g):
    """(root int32 [N], size int32 [N]) by a plain union-find over undirected same-label edges: root = the component's smallest
    index, size = its point count at roots, 0 elsewhere."""
    parent = list(range(g.n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i in range(g.n):
        for j in g.neighbours(i):
            if g.label[j] == g.label[i]:
                a, b = find(i), find(int(j))
                if a != b:
                    parent[max(a, b)] = min(a, b)
    root = np.array([find(i) for i in range(g.n)], dtype=np.int32).reshape(-1)
    size = np.zeros(g.n, dtype=np.int32)
    np.add.at(size, root, 1)
    return root, size


def component_clusters(root, size, threshold):
    """Clusters of the components: ascending root, ascending points inside."""
    return [np.nonzero(root == r)[0].tolist() for r in np.nonzero((root == np.arange(root.shape[0])) & (size >= threshold))[0]]


def pack_clusters(clusters):
    """(cluster_idxs int32 [sum, 2], cluster_offsets int32 [nCluster + 1])"""
    idxs = np.array([(c, p) for c, pts in enumerate(clusters) for p in pts], dtype=np.int32).reshape(-1, 2)
    offsets = np.cumsum([0] + [len(pts) for pts in clusters]).astype(np.int32)
    return idxs, offsets


def unpack_clusters(idxs, offsets):
    idxs, offsets = np.asarray(idxs), np.asarray(offsets)
    assert idxs.shape[0] == offsets[-1] and offsets[0] == 0
    out = []
    for c in range(offsets.shape[0] - 1):
        rows = idxs[offsets[c]:offsets[c + 1]]
        assert (rows[:, 0] == c).all()
        out.append(rows[:, 1].tolist())
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# segment pools
# ---------------------------------------------------------------------------------------------------------------------------
def seg_ranges(offsets, n_rows):
    o = np.clip(np.asarray(offsets, dtype=np.int64), 0, n_rows)
    return [(int(a), int(max(a, b))) for a, b in zip(o[:-1], o[1:])]


def sec_mean(inp, offsets):
    """fp32, the quotient rounded, then added, in index order."""
    out = np.zeros((len(offsets) - 1, inp.shape[1]), dtype=F32)
    with np.errstate(all="ignore"):
        for s, (lo, hi) in enumerate(seg_ranges(offsets, inp.shape[0])):
            count = F32(hi - lo)
            acc = np.zeros(inp.shape[1], dtype=F32)
            for r in range(lo, hi):
                acc = (acc + (inp[r] / count).astype(F32)).astype(F32)
            out[s] = acc
    return out


def sec_mean_bound(inp, offsets):
    """(float64 mean, bound): |out - mean| <= (len + 2) * 2^-24 * sum|x| / len per channel — len rounded quotients and len - 1
    rounded additions, to first order, in whatever order the additions come."""
    ns, c = len(offsets) - 1, inp.shape[1]
    ref, bound = np.zeros((ns, c)), np.zeros((ns, c))
    with np.errstate(all="ignore"):
        for s, (lo, hi) in enumerate(seg_ranges(offsets, inp.shape[0])):
            if hi > lo:
                x = inp[lo:hi].astype(np.float64)
                ref[s] = x.sum(0) / (hi - lo)
                bound[s] = (hi - lo + 2) * 2.0 ** -24 * np.abs(x).sum(0) / (hi - lo)
    return ref, bound


def check_sec_mean(out, inp, offsets):
    """Assert the bound where the float64 mean is finite, and the same non-finite value elsewhere."""
    ref, bound = sec_mean_bound(inp, offsets)
    fin = np.isfinite(ref)
    with np.errstate(all="ignore"):
        err = np.abs(out.astype(np.float64) - ref)
    assert (err[fin] <= bound[fin]).all(), float((err[fin] - bound[fin]).max())
    with np.errstate(all="ignore"):
        assert np.array_equal(out[~fin], ref[~fin].astype(F32), equal_nan=True)
    return float((err[fin] / np.maximum(bound[fin], 1e-300)).max()) if fin.any() else 0.0


def _extreme(inp, offsets, sign):
    """Sequential strict compare from -inf (max: sign = 1) or +inf (min: sign = -1): (value, smallest row that holds it or -1)."""
    ns, c = len(offsets) - 1, inp.shape[1]
    val = np.full((ns, c), -sign * np.inf, dtype=F32)
    arg = np.full((ns, c), -1, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for s, (lo, hi) in enumerate(seg_ranges(offsets, inp.shape[0])):
            for r in range(lo, hi):
                win = inp[r] > val[s] if sign > 0 else inp[r] < val[s]
                val[s] = np.where(win, inp[r], val[s])
                arg[s] = np.where(win, r, arg[s])
    return val, arg


def sec_max(inp, offsets):
    return _extreme(inp, offsets, 1)[0]


def sec_min(inp, offsets):
    return _extreme(inp, offsets, -1)[0]


def roipool(inp, offsets):
    return _extreme(inp, offsets, 1)


def sec_mean_bp(d_out, offsets, n_rows):
    d_inp = np.zeros((n_rows, d_out.shape[1]), dtype=F32)
    for s, (lo, hi) in enumerate(seg_ranges(offsets, n_rows)):
        if hi > lo:
            d_inp[lo:hi] = (d_out[s] / F32(hi - lo)).astype(F32)
    return d_inp


def roipool_bp(d_out, maxidx, n_rows):
    d_feats = np.zeros((n_rows, d_out.shape[1]), dtype=F32)
    for s in range(d_out.shape[0]):
        for ch in range(d_out.shape[1]):
            if 0 <= maxidx[s, ch] < n_rows:
                d_feats[maxidx[s, ch], ch] += d_out[s, ch]
    return d_feats


SEG_LENGTHS = (0, 1, 63, 64, 65, 5000)
SEG_CHANNELS = (1, 16, 33)
SEG_LEAD, SEG_TAIL = 3, 4     # rows before the first and after the last segment: outside every segment


def seg_case(c, seed=0):
    """(inp [rows, c], offsets): the lengths of SEG_LENGTHS in one offsets array, rows outside every segment at both ends, and in
    channel 0 / c - 1: a column of all -inf (the 64-row segment), a NaN (the 5000-row one), ties for the maximum and the minimum
    (the 65-row one), zeros of both signs (the 63-row one)."""
    rng = np.random.default_rng(1000 + 17 * c + seed)
    offsets = (SEG_LEAD + np.cumsum((0,) + SEG_LENGTHS)).astype(np.int32)
    inp = rng.standard_normal((int(offsets[-1]) + SEG_TAIL, c)).astype(F32)
    o = {l: int(offsets[k]) for k, l in enumerate(SEG_LENGTHS)}
    inp[o[64]:o[64] + 64, 0] = -np.inf
    inp[o[5000] + 1234, 0] = np.nan
    inp[o[65] + 9, c - 1] = inp[o[65] + 40, c - 1] = inp[o[65] + 64, c - 1] = 100.0
    inp[o[65] + 3, c - 1] = inp[o[65] + 30, c - 1] = -100.0
    inp[o[63]:o[63] + 63, c - 1] = 0.0
    inp[o[63] + 5:o[63] + 63:2, c - 1] = -0.0
    return inp, offsets


LONG_SEGMENT = 2048     # DODA_PG_LONG_SEGMENT: rows per segment on average from which the kernels run 1024-thread workgroups


def seg_case_long(c, seed=3):
    """Segments of 9000, 1 and 0 rows — 3000 rows per segment on average, the other workgroup size of the kernels — with equal
    maxima 7995 rows apart (rows of different waves), a NaN, and rows outside every segment at both ends."""
    rng = np.random.default_rng(5000 + 17 * c + seed)
    offsets = (SEG_LEAD + np.cumsum((0, 9000, 1, 0))).astype(np.int32)
    inp = rng.standard_normal((int(offsets[-1]) + SEG_TAIL, c)).astype(F32)
    inp[SEG_LEAD + 8000, c - 1] = inp[SEG_LEAD + 5, c - 1] = 100.0
    inp[SEG_LEAD + 4000, 0] = np.nan
    assert inp.shape[0] >= LONG_SEGMENT * 3
    return inp, offsets


def seg_case_many(c=16, n_seg=33000, seed=1):
    """33000 segments of one row each."""
    rng = np.random.default_rng(2000 + seed)
    return rng.standard_normal((n_seg, c)).astype(F32), np.arange(n_seg + 1, dtype=np.int32)


def seg_case_corrupt(c=16, seed=2):
    """Offsets that go backwards and leave the array: segments (clamped) [0,4) [4,2)=empty [2,20) [20,rows) [rows,11)=empty."""
    rng = np.random.default_rng(3000 + seed)
    inp = rng.standard_normal((40, c)).astype(F32)
    return inp, np.array([-5, 4, 2, 20, 47, 11], dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# proposal IoU
# ---------------------------------------------------------------------------------------------------------------------------
IOU_INSTANCES = (1, 37, 300)


def iou_case(n_instance, n_points=3000, seed=0):
    """(proposals_idx int32, proposals_offset int32, instance_labels int64 [n_points], instance_pointnum int32 [n_instance]).
    Labels include -100, another negative, n_instance itself and a value past 2^32; proposals include an empty one, one inside
    a single instance, and one holding point indices outside [0, n_points)."""
    rng = np.random.default_rng(4000 + n_instance + seed)
    labels = rng.integers(0, n_instance, n_points).astype(np.int64)
    labels[rng.random(n_points) < 0.2] = -100
    labels[5], labels[6], labels[7] = -3, n_instance, 2 ** 32 + (n_instance - 1)
    labels[8] = n_instance - 1
    pointnum = np.bincount(labels[(labels >= 0) & (labels < n_instance)], minlength=n_instance).astype(np.int32)
    props = [rng.choice(n_points, size=int(k), replace=False) for k in (700, 1, 300, 64)]
    props.insert(2, np.zeros(0, dtype=np.int64))                                        # an empty proposal
    props.append(np.nonzero(labels == n_instance - 1)[0])                               # every point inside one instance
    props.append(np.concatenate(([-1, n_points, 2 ** 31 - 1, -2 ** 31], np.arange(5, 60))))   # corrupt point indices, odd labels
    idx = np.concatenate(props).astype(np.int64).astype(np.int32)
    offset = np.cumsum([0] + [len(p) for p in props]).astype(np.int32)
    return idx, offset, labels, pointnum


def get_iou(idx, offset, labels, pointnum):
    n_instance, n_points = pointnum.shape[0], labels.shape[0]
    out = np.zeros((len(offset) - 1, n_instance), dtype=F32)
    for p, (lo, hi) in enumerate(seg_ranges(offset, idx.shape[0])):
        ids = idx[lo:hi].astype(np.int64)
        labs = labels[ids[(ids >= 0) & (ids < n_points)]]
        inter = np.bincount(labs[(labs >= 0) & (labs < n_instance)], minlength=n_instance).astype(np.int64)
        union = (hi - lo) + pointnum.astype(np.int64) - inter
        out[p] = (inter.astype(F32).astype(np.float64) / (union.astype(F32).astype(np.float64) + 1e-5)).astype(F32)
    return out
