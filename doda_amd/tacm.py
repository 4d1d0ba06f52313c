"""Tail-aware cuboid mixing (TACM) of the self-training stage on the device (reference dataset/augmentor/augmentor_utils.py:255-445,
dataset/augmentor/data_augmentor.py:15-108, dataset/mix_dataset.py:59-82).

Every target sample is cut into split[0] x split[1] x split[2] cuboids by randomly placed planes, about `mix_ratio` of them are
replaced by cuboids of a source scene, the cuboids are permuted, and target cuboids that lack tail classes are replaced from a
class-balanced queue of earlier tail-class cuboids.  The reference does this per sample with numpy boolean masks in DataLoader
workers; here the scenes stay on the device:

  device (include/doda_mix.h)   bounds -> classify + statistics -> emit (stable compaction + transform) -> extract (queue cuboids)
  host (this file, numpy fp64)  the planes (split_planes), the mixing plan (plan_sample) and the sampler (SplitSampler) — a few
                                hundred bytes per sample, drawn from one `draws` object in the reference's order

Two deliberate deviations: queue cuboids are immutable (the reference moves and shrinks a stored cuboid in place every
time it is drawn, so it shrinks by 10 % per use; here the transform is applied in the emit kernel: the first use is identical), and
every rank keeps its own queue (the reference all-gathers pickled cuboids)."""
import threading

import numpy as np
import torch

from . import _lib, segments
from ._lib import check, lib
from .segments import SeededDraws, launch_on, offsets_h, per_sample, stream_handle   # noqa: F401  (SeededDraws: for the callers)

FIX = float(1 << _lib.MIX_FIXED_BITS)
MAX_EXTENT = 2048.0          # metres: |centred coordinate| * 2^28 * points of a cuboid stays inside int64


# ------------------------------------------------------------------------------------------------ configuration
class TacmConfig:
    """DATA_CONFIG_TAR.DATA_AUG.tacm with the reference's keys and defaults (cfgs/dataset_cfgs/scannet/scannet_cfg.yaml:45-58);
    an absent section is a disabled one.  class_ratio / class_thres / tail_class_idx are set by SplitSampler.update_cfg."""

    def __init__(self, enabled=False, split=(2, 2, 1), p=0.5, mix_ratio=0.5, permute_enabled=True, permute_p=0.5, queue_enabled=True,
                 queue_size=256, num_cuboid=2.0, num_class=2, update_class_ratio=True, n_classes=20):
        self.enabled, self.split, self.p, self.mix_ratio = bool(enabled), [int(v) for v in split], p, float(mix_ratio)
        self.permute_enabled, self.permute_p = bool(permute_enabled), permute_p
        self.queue_enabled, self.queue_size, self.num_cuboid = bool(queue_enabled), int(queue_size), float(num_cuboid)
        self.num_class, self.update_class_ratio, self.n_classes = int(num_class), bool(update_class_ratio), int(n_classes)
        self.class_ratio = self.class_thres = self.tail_class_idx = None
        if len(self.split) != 3 or min(self.split) < 1:
            raise ValueError("tacm.split: three positive integers")
        if self.total_splits > _lib.MIX_MAX_CUBOIDS:
            raise ValueError("tacm.split: at most %d cuboids" % _lib.MIX_MAX_CUBOIDS)
        if not 1 <= self.n_classes <= _lib.MIX_MAX_CLASSES:
            raise ValueError("tacm: 1..%d classes" % _lib.MIX_MAX_CLASSES)

    @property
    def total_splits(self):
        return self.split[0] * self.split[1] * self.split[2]

    @classmethod
    def from_section(cls, sec, n_classes=20):
        if sec is None:
            return cls(enabled=False, n_classes=n_classes)
        pc, cq = sec.get("permute_cuboid", {}) or {}, sec.get("cuboid_queue", {}) or {}
        return cls(enabled=sec.get("enabled", True), split=sec.get("split", [2, 2, 1]), p=sec.get("p", None),
                   mix_ratio=sec.get("mix_ratio", 0.5), permute_enabled=pc.get("enabled", True), permute_p=pc.get("p", None),
                   queue_enabled=cq.get("enabled", False), queue_size=cq.get("size", 256), num_cuboid=cq.get("num_cuboid", 2.0),
                   num_class=cq.get("num_class", 2), update_class_ratio=cq.get("update_class_ratio", True), n_classes=n_classes)

    @classmethod
    def from_cfg(cfg_cls, cfg):
        """From an experiment config: DATA_CONFIG_TAR.DATA_AUG.tacm (absent = disabled = the unmixed target loader)."""
        n_classes = int(cfg.COMMON_CLASSES.n_classes) if "COMMON_CLASSES" in cfg else 20
        sec = None
        if "DATA_CONFIG_TAR" in cfg and "DATA_AUG" in cfg.DATA_CONFIG_TAR and "tacm" in cfg.DATA_CONFIG_TAR.DATA_AUG:
            sec = cfg.DATA_CONFIG_TAR.DATA_AUG.tacm
        return cfg_cls.from_section(sec, n_classes)


# ------------------------------------------------------------------------------------------------ randomness
class ReplayDraws:
    """Replays a recorded draw sequence [(kind, value), ...] and checks that the draws are asked for in the recorded order."""

    def __init__(self, record):
        self.record, self.pos = list(record), 0

    def _next(self, kind):
        if self.pos >= len(self.record) or self.record[self.pos][0] != kind:
            raise AssertionError("draw %d: %s asked, %s recorded" % (
                self.pos, kind, self.record[self.pos][0] if self.pos < len(self.record) else "nothing"))
        self.pos += 1
        return self.record[self.pos - 1][1]

    def rand(self, n=None):
        v = np.asarray(self._next("rand"), dtype=np.float64)
        if (n is None) != (v.ndim == 0) or (n is not None and v.shape != (n,)):
            raise AssertionError("draw %d: rand(%s) asked, shape %s recorded" % (self.pos - 1, n, v.shape))
        return float(v) if n is None else v

    def permutation(self, n):
        v = np.asarray(self._next("permutation"), dtype=np.int64)
        assert v.shape == (n,)
        return v

    def choice(self, n, k, p):
        v = np.asarray(self._next("choice"), dtype=np.int64)
        assert v.shape == (k,) and (v < n).all()
        return v

    def sample(self, k, n):
        v = [int(x) for x in np.atleast_1d(self._next("sample"))]
        assert len(v) == k and all(x < n for x in v)
        return v

    def exhausted(self):
        return self.pos == len(self.record)


# ------------------------------------------------------------------------------------------------ the queue
class Cuboid:
    """One queue item: the centred, unmixed points of a tail-class target cuboid as fp32 rows (x, y, z, label) [n, 4] — a device
    tensor in the queue, a CPU tensor in split_sampler.pth — with what the plan needs of it: the coordinate maximum, the
    coordinate sums (fp64) and the label histogram."""

    def __init__(self, rows, cmax=None, csum=None, hist=None, n_classes=20):
        self.rows = rows
        if cmax is None or csum is None or hist is None:
            h = rows.detach().cpu().numpy()
            cmax = h[:, :3].max(0)
            csum = h[:, :3].astype(np.float64).sum(0)
            hist = label_histogram(h[:, 3], n_classes)
        self.max = np.asarray(cmax, dtype=np.float32)
        self.sum = np.asarray(csum, dtype=np.float64)
        self.hist = np.asarray(hist, dtype=np.int64)

    @property
    def n(self):
        return int(self.rows.shape[0])


def label_histogram(labels, n_classes):
    """np.histogram(labels, bins=np.arange(n_classes + 1))[0] for integer-valued labels: counts of 0 .. n_classes - 1, the last
    bin closed (a label equal to n_classes counts there), anything else dropped."""
    lab = np.asarray(labels).astype(np.int64)
    h = np.bincount(lab[(lab >= 0) & (lab < n_classes)], minlength=n_classes).astype(np.int64)
    h[n_classes - 1] += int((lab == n_classes).sum())
    return h


class Queue:
    """Ring buffer of data_augmentor.py:15-40."""

    def __init__(self, size):
        assert size > 0
        self.size, self.queue, self.ptr, self.cur_size, self.got = size, [None] * size, 0, 0, 0

    def update_queue(self, items):
        if len(items) == 0:
            return
        items = list(items)[:self.size]
        for it in items:                       # (the reference's two slice assignments: from ptr on, wrapping to the front)
            self.queue[self.ptr] = it
            self.ptr = (self.ptr + 1) % self.size
        self.cur_size = min(self.cur_size + len(items), self.size)

    def get_item(self, n, draws):
        if self.cur_size == 0:
            return []
        n = min(n, self.cur_size)
        items = [self.queue[i] for i in draws.sample(n, self.cur_size)]
        self.got += n
        return items


class SplitSampler:
    """The class-balanced queue of tail-class cuboids (data_augmentor.py:43-108), with the reference's state and arithmetic.
    The loader thread draws from it while the training thread updates it: one lock around both."""

    def __init__(self, cfg):
        self.total_size, self.num_c, self.n_classes = cfg.queue_size, cfg.num_class, cfg.n_classes
        self.lock = threading.Lock()

    def init_finish(self):
        return hasattr(self, "class_ratio")

    def init_class_ratio(self, class_ratio):
        self.class_ratio = np.asarray(class_ratio, dtype=np.float64)
        mask = self.class_ratio > 0
        with np.errstate(divide="ignore"):
            self.inverse_class_ratio = np.where(mask, 1.0 / (self.class_ratio + 10e-10), 10e-10)
        self.tail_class_ratio = np.sort(-self.inverse_class_ratio)[:self.num_c]
        self.tail_class_ratio /= self.tail_class_ratio.sum()
        self.tail_class_idx = np.argsort(-self.inverse_class_ratio)[:self.num_c]
        self.queues = [Queue(max(1, int(self.total_size * self.tail_class_ratio[c]))) for c in range(self.num_c)]

    def update_cfg(self, cfg):
        cfg.class_ratio = self.class_ratio
        cfg.class_thres = np.ones_like(cfg.class_ratio)
        cfg.class_thres[self.tail_class_idx] = self.class_ratio[self.tail_class_idx]
        cfg.tail_class_idx = self.tail_class_idx

    def _need_init(self):
        if not self.init_finish():
            raise ValueError("Split sampler is not inited! (init_class_ratio from pseudo_labels/class_ratio.txt: python -m doda_amd.st)")

    def update(self, items):
        self._need_init()
        assert len(items) == self.num_c
        with self.lock:
            for c in range(self.num_c):
                self.queues[c].update_queue(items[c])

    def get_split(self, n, draws):
        self._need_init()
        if n == 0:
            return []
        with self.lock:
            items = []
            for c in draws.choice(self.num_c, n, self.tail_class_ratio):
                items.extend(self.queues[int(c)].get_item(1, draws))
            return items

    def update_class_ratio(self, class_ratio):
        class_ratio = np.asarray(class_ratio, dtype=np.float64)
        if class_ratio.max() > 0.0:
            inverse = 1.0 / (class_ratio + 10e-1)
            inverse /= inverse.sum()
            with self.lock:
                self.tail_class_ratio = 0.999 * self.tail_class_ratio + 0.001 * inverse

    def save_sampler(self, path):
        with self.lock:
            queues = [{"size": q.size, "ptr": q.ptr, "cur_size": q.cur_size, "got": q.got,
                       "queue": [None if it is None else it.rows.detach().cpu() for it in q.queue]} for q in self.queues]
            torch.save({"queues": queues, "class_ratio": self.class_ratio, "inverse_class_ratio": self.inverse_class_ratio,
                        "tail_class_ratio": self.tail_class_ratio, "tail_class_idx": self.tail_class_idx}, path)

    def load_sampler(self, path, device=None):
        buf = torch.load(path, map_location="cpu", weights_only=False)
        queues = []
        for d in buf["queues"]:
            q = Queue(d["size"])
            q.ptr, q.cur_size, q.got = d["ptr"], d["cur_size"], d["got"]
            q.queue = [None if r is None else Cuboid(r.to(device) if device is not None else r, n_classes=self.n_classes)
                       for r in d["queue"]]
            queues.append(q)
        with self.lock:
            self.queues = queues
            self.class_ratio, self.inverse_class_ratio = buf["class_ratio"], buf["inverse_class_ratio"]
            self.tail_class_ratio, self.tail_class_idx = buf["tail_class_ratio"], buf["tail_class_idx"]


# ------------------------------------------------------------------------------------------------ the plan (host, fp64)
def centre_of(bounds):
    """bounds fp32 [2, 3] (min, max of the raw scene) -> (centre, centred min, centred max), fp32 as augmentor_utils.py:259-260:
    the centred extremes are the extremes of the centred points because the fp32 subtraction is monotone."""
    b = np.asarray(bounds, dtype=np.float32)
    c = (b[0] + b[1]) / np.float32(2.0)
    return c, b[0] - c, b[1] - c


def split_planes(cmin, cmax, split, draws):
    """split_space (augmentor_utils.py:422-441): (split_coord, split_range) fp64 [total, 3] — the upper corner and the extent of
    every cuboid — from the centred fp32 extremes.  One draw per axis, split or not."""
    cmin, cmax = np.asarray(cmin, dtype=np.float32), np.asarray(cmax, dtype=np.float32)
    if not np.all(np.isfinite(cmin)) or float(np.max(cmax - cmin)) > MAX_EXTENT:
        raise ValueError("tacm: a scene needs finite coordinates within %g m" % MAX_EXTENT)
    rng32 = (cmax - cmin) + np.float32(0.001)                             # fp32
    ratio, ratio_range = [], []
    for k in range(3):
        step = float(np.float32(1.0) / np.float32(split[k]))              # the fp32 reciprocal, widened
        r = np.cumsum(np.array([step] * split[k], dtype=np.float64))
        r = np.append(r[:-1] + (draws.rand() - 0.5) * 0.2, 1.0)
        ratio.append(r)
        ratio_range.append(np.append(r[0], r[1:] - r[:-1]))
    total = split[0] * split[1] * split[2]
    coord, rng = np.empty((total, 3), dtype=np.float64), np.empty((total, 3), dtype=np.float64)
    for i in range(total):
        idx = (i // (split[1] * split[2]), i % (split[1] * split[2]) // split[2], i % split[2])
        for k in range(3):
            coord[i, k] = ratio[k][idx[k]] * float(rng32[k]) + float(cmin[k])
            rng[i, k] = ratio_range[k][idx[k]] * float(rng32[k])
    return coord, rng


def split_status_of(hist, cfg):
    """Per cuboid (augmentor_utils.py:375-383) from its label histogram [total, n_classes + 1] (last bin: ignored labels):
    status [total, num_class] — which tail classes exceed their threshold in the cuboid.  A cuboid without points, or with
    ignored labels only, has none."""
    total = hist.shape[0]
    status = np.zeros((total, cfg.num_class), dtype=bool)
    if not cfg.queue_enabled:
        return status
    for s in range(total):
        counted = hist[s, :cfg.n_classes]
        if counted.sum() > 0:
            ratio = counted / 1.0 / counted.sum()                        # np.histogram(..., density=True) with unit bins
            status[s] = (ratio > cfg.class_thres)[cfg.tail_class_idx]
    return status


class SamplePlan:
    """What the emit / extract kernels need for one (target, source) pair, and what the reference's tacm() returns beside the
    points."""


def begin_sample(bounds_t, bounds_s, cfg, draws):
    """First half of the plan: the centring and the cuboid planes of the target and then the source scene (three draws each)."""
    p = SamplePlan()
    p.centre_t, tmin, tmax = centre_of(bounds_t)
    p.centre_s, smin, smax = centre_of(bounds_s)
    p.coord_t, p.range_t = split_planes(tmin, tmax, cfg.split, draws)
    p.coord_s, p.range_s = split_planes(smin, smax, cfg.split, draws)
    return p


def planes_of(coord, rng):
    """[total, 2, 3]: (hi, lo) of doda_mix_classify — x < hi and x >= hi - range (augmentor_utils.py:444-445)."""
    return np.stack((coord, coord - rng), 1)


def _group(stats_seg, o, total):
    """(count, fp64 coordinate sum) of the points that move with cuboid o: its own and, for the last cuboid, those of no cuboid
    (the reference indexes its mappers with their id -1, i.e. the last entry)."""
    n = int(stats_seg[o, 3:].sum())
    sx = stats_seg[o, :3].astype(np.float64)
    if o == total - 1:
        n += int(stats_seg[total, 3:].sum())
        sx = sx + stats_seg[total, :3].astype(np.float64)
    return n, sx / FIX


def finish_sample(p, stats_t, stats_s, cfg, sampler, draws):
    """Second half (augmentor_utils.py:269-364) from the statistics int64 [total + 1, 3 + n_classes + 1] of the two scenes
    (doda_mix_classify): fills keep / shift / shrink per cuboid, the queue cuboids chosen with their transforms, the sample's
    mean, the output sizes, tar_tail_splits (cuboid ids per tail class) and tar_splits_class_ratio."""
    total = cfg.total_splits
    hist_t = stats_t[:total, 3:]
    status = split_status_of(hist_t, cfg)
    p.tail_splits = [[int(s) for s in np.nonzero(status[:, i])[0]] for i in range(cfg.num_class)]
    split_status = status.any(1)
    p.split_status0 = split_status.copy()
    # cuboid mixing: 1 source, 0 target
    concat = cfg.p is None or draws.rand() < cfg.p
    concat_seq = (draws.rand(total) < cfg.mix_ratio).astype(np.int64) if concat else np.zeros(total, dtype=np.int64)
    n_src = int(concat_seq.sum())
    n_tar = total - n_src
    tar_slots, src_slots = np.nonzero(concat_seq == 0)[0], np.nonzero(concat_seq == 1)[0]
    p.permute = cfg.permute_p is None or draws.rand() < cfg.permute_p
    if p.permute:
        p.perm_t, p.perm_s = draws.permutation(total), draws.permutation(total)
        order_t, order_s = p.perm_t[:n_tar], p.perm_s[:n_src]
    else:
        p.perm_t = p.perm_s = None
        order_t, order_s = tar_slots, src_slots
    split_status = split_status[order_t]
    # cuboids from the queue replace the LAST target slots
    items = []
    if cfg.queue_enabled:
        n_eligible = int((cfg.num_cuboid // 1) + int(draws.rand() < cfg.num_cuboid % 1))
        supp = min(n_tar, n_eligible) - int(split_status.sum())
        if supp > 0:
            items = sampler.get_split(supp, draws)
    n_q = len(items)
    p.concat_seq, p.split_status, p.items = concat_seq, split_status, items
    p.kept_t, p.kept_s = [int(o) for o in order_t[:n_tar - n_q]], [int(o) for o in order_s]
    # per cuboid: keep, shift, shrink; the sample's mean from the groups' means
    p.tab_t, p.tab_s = np.zeros((total + 1, 7)), np.zeros((total + 1, 7))
    weighted, n_out = np.zeros(3), 0
    p.n_t = p.n_s = 0
    for tab, kept, slots, coord, stats, which in ((p.tab_t, p.kept_t, tar_slots, p.coord_t, stats_t, "t"),
                                                  (p.tab_s, p.kept_s, src_slots, p.coord_s, stats_s, "s")):
        for j, o in enumerate(kept):
            n, sx = _group(stats, o, total)
            shift = coord[slots[j]] - coord[o] if p.permute else np.zeros(3)
            tab[o, 0], tab[o, 1:4] = 1.0, shift
            if n > 0:
                mean = sx / n + shift
                tab[o, 4:7] = -mean * 0.1
                weighted += n * (mean * 0.9)
            n_out += n
            if which == "t":
                p.n_t += n
            else:
                p.n_s += n
        tab[total] = tab[total - 1]                                      # points of no cuboid go with the last one
    p.item_tab = np.zeros((n_q, 7))
    for q, it in enumerate(items):
        shift = p.coord_t[tar_slots[n_tar - n_q + q]] - it.max.astype(np.float64)
        mean = it.sum / max(it.n, 1) + shift
        p.item_tab[q, 0], p.item_tab[q, 1:4], p.item_tab[q, 4:7] = 1.0, shift, -mean * 0.1
        weighted += it.n * (mean * 0.9)
        n_out += it.n
    p.n_out = n_out
    p.mean = weighted / n_out if n_out > 0 else np.zeros(3)
    if cfg.queue_enabled:
        h = np.zeros(cfg.n_classes, dtype=np.int64)
        for it in items:
            h += it.hist
        p.class_ratio = h[cfg.tail_class_idx]
    else:
        p.class_ratio = np.zeros(3)
    return p


def plan(bounds, stats, cfg, sampler, draws):
    """The whole plan of ONE sample on the host.  bounds fp32 [2][2, 3]: (min, max) of the raw target and source scene; stats:
    a function (planes_t, planes_s) -> (stats_t, stats_s) (the classify pass between the two halves), or that pair itself when
    the statistics for these draws' planes are known already."""
    p = begin_sample(bounds[0], bounds[1], cfg, draws)
    if callable(stats):
        stats = stats(planes_of(p.coord_t, p.range_t), planes_of(p.coord_s, p.range_s))
    return finish_sample(p, np.asarray(stats[0]), np.asarray(stats[1]), cfg, sampler, draws)


# ------------------------------------------------------------------------------------------------ device calls
def n_blocks(offsets):
    return segments.n_blocks(lib(), "doda_mix_blocks", offsets)


def segment_bounds(xyz, offsets, stream=None):
    """fp32 [n_seg, 2, 3] device tensor: per segment (min, max) of the rows' first three columns (doda_mix_bounds).  Segments
    are taken MIX_MAX_SEGMENTS at a time."""
    assert xyz.is_cuda and xyz.dtype == torch.float32 and xyz.is_contiguous() and xyz.dim() == 2 and xyz.shape[1] in (3, 4)
    n_seg = len(offsets) - 1
    out = torch.empty((n_seg, 2, 3), dtype=torch.float32, device=xyz.device)
    for s0 in range(0, n_seg, _lib.MIX_MAX_SEGMENTS):
        s1 = min(n_seg, s0 + _lib.MIX_MAX_SEGMENTS)
        sub = [int(v) - int(offsets[s0]) for v in offsets[s0:s1 + 1]]
        arr, ns = offsets_h(sub)
        part = torch.empty((max(1, n_blocks(sub)), 6), dtype=torch.float32, device=xyz.device)
        check(lib().doda_mix_bounds(xyz[int(offsets[s0]):].data_ptr(), xyz.shape[1], arr, ns, part.data_ptr(), out[s0:].data_ptr(),
                                    stream_handle(stream)), "doda_mix_bounds")
    return out


def classify(xyz, labels, offsets, centre, planes, n_classes, stream=None):
    """(cub uint8 [N], stats int64 [n_seg, n_cub + 1, 3 + n_classes + 1], blk_cnt int32 [blocks, n_cub + 1]) (doda_mix_classify).
    centre fp32 [n_seg, 3], planes fp64 [n_seg, n_cub, 2, 3], device tensors."""
    n_seg, n_cub = planes.shape[0], planes.shape[1]
    assert xyz.dtype == torch.float32 and labels.dtype == torch.int32 and centre.dtype == torch.float32 and planes.dtype == torch.float64
    assert xyz.is_contiguous() and labels.is_contiguous() and centre.is_contiguous() and planes.is_contiguous()
    assert n_seg == len(offsets) - 1 and int(offsets[-1]) == xyz.shape[0] == labels.shape[0] and centre.shape == (n_seg, 3)
    dev = xyz.device
    cub = torch.empty(xyz.shape[0], dtype=torch.uint8, device=dev)
    stats = torch.zeros((n_seg, n_cub + 1, 3 + n_classes + 1), dtype=torch.int64, device=dev)
    blk_cnt = torch.empty((max(1, n_blocks(offsets)), n_cub + 1), dtype=torch.int32, device=dev)
    arr, ns = offsets_h(offsets)
    check(lib().doda_mix_classify(xyz.data_ptr(), labels.data_ptr(), arr, ns, centre.data_ptr(), planes.data_ptr(), n_cub, n_classes,
                                  cub.data_ptr(), stats.data_ptr(), blk_cnt.data_ptr(), stream_handle(stream)), "doda_mix_classify")
    return cub, stats, blk_cnt


def _emit(xyz, labels, cub, blk_cnt, offsets, n_cub, centre, tab, seg_tab, out, stream):
    arr, ns = offsets_h(offsets)
    dev = xyz.device
    tab_d = torch.from_numpy(np.ascontiguousarray(tab, dtype=np.float64)).to(dev)
    seg_d = torch.from_numpy(np.ascontiguousarray(seg_tab, dtype=np.float64)).to(dev)
    check(lib().doda_mix_emit(xyz.data_ptr(), xyz.shape[1], labels.data_ptr() if labels is not None else None,
                              cub.data_ptr() if cub is not None else None, blk_cnt.data_ptr() if blk_cnt is not None else None,
                              arr, ns, n_cub, centre.data_ptr() if centre is not None else None, tab_d.data_ptr(), seg_d.data_ptr(),
                              out["xyz_mid"].data_ptr(), out["labels"].data_ptr(), out["mask1"].data_ptr(), out["mask2"].data_ptr(),
                              out["xyz_mid"].shape[0], stream_handle(stream)), "doda_mix_emit")


def extract(xyz, labels, cub, blk_cnt, offsets, n_cub, centre, ex_base, n_rows, stream=None):
    """fp32 [n_rows, 4]: the centred points (x, y, z, label) of the wanted cuboids, cuboid (s, c) from row ex_base[s][c]
    (doda_mix_extract).  ex_base: int64 numpy [n_seg, n_cub + 1], negative = not wanted."""
    arr, ns = offsets_h(offsets)
    rows = torch.empty((n_rows, 4), dtype=torch.float32, device=xyz.device)
    ex_d = torch.from_numpy(np.ascontiguousarray(ex_base, dtype=np.int64)).to(xyz.device)
    check(lib().doda_mix_extract(xyz.data_ptr(), labels.data_ptr(), cub.data_ptr(), blk_cnt.data_ptr(), arr, ns, n_cub,
                                 centre.data_ptr(), ex_d.data_ptr(), rows.data_ptr(), n_rows, stream_handle(stream)), "doda_mix_extract")
    return rows


@torch.no_grad()
def mix_batch(target_xyz, target_labels, target_offsets, source_xyz, source_labels, source_offsets, cfg, sampler, draws, stream=None,
              return_debug=False):
    """Mix a batch: sample b = target segment b + source segment b (reference tacm(), augmentor_utils.py:255-365, per sample).

    target_xyz / source_xyz fp32 [N, 3], *_labels int32 [N], *_offsets B + 1 host integers; draws: one draws object per sample
    (or one object, for a batch of one) — rand(), permutation(n), choice(n, k, p), sample(k, n), consumed in the reference's
    order.  `stream`: the stream to launch on (default: torch's current stream; the two small read-backs block the calling
    thread only — the loader thread).
    -> dict: xyz_mid fp32 [M, 3], labels int32 [M], offsets (B + 1 integers), mask1 / mask2 bool [M], tar_tail_splits (list,
    num_class entries per sample, each a list of Cuboid), tar_splits_class_ratio (summed over the samples, as the reference's
    collate_fn does)."""
    if not cfg.enabled:
        raise ValueError("mix_batch: tacm is disabled in this configuration")
    if cfg.queue_enabled and cfg.class_thres is None:
        raise ValueError("mix_batch: the split sampler's thresholds are missing (SplitSampler.init_class_ratio + update_cfg)")
    dev = target_xyz.device
    B = len(target_offsets) - 1
    if len(source_offsets) - 1 != B:
        raise ValueError("mix_batch: one source scene per target scene")
    draws = per_sample(draws, B, "mix_batch")
    with launch_on(stream):
        total, K = cfg.total_splits, cfg.n_classes
        nt = int(target_offsets[-1])
        xyz = torch.cat((target_xyz, source_xyz), 0).contiguous()
        labels = torch.cat((target_labels, source_labels), 0).to(torch.int32).contiguous()
        offsets = [int(v) for v in target_offsets] + [nt + int(v) for v in source_offsets[1:]]
        bounds = segment_bounds(xyz, offsets, stream).cpu().numpy()                          # read-back 1: 24 B per segment
        plans = [begin_sample(bounds[b], bounds[B + b], cfg, draws[b]) for b in range(B)]
        centre = np.stack([p.centre_t for p in plans] + [p.centre_s for p in plans]).astype(np.float32)
        planes = np.stack([planes_of(p.coord_t, p.range_t) for p in plans] + [planes_of(p.coord_s, p.range_s) for p in plans])
        centre_d, planes_d = torch.from_numpy(centre).to(dev), torch.from_numpy(planes).to(dev)
        cub, stats_d, blk_cnt = classify(xyz, labels, offsets, centre_d, planes_d, K, stream)
        stats = stats_d.cpu().numpy()                                                        # read-back 2: counts, histograms, sums
        tab = np.zeros((2 * B, total + 1, 7))
        seg_tab = np.zeros((2 * B, 5))
        out_offsets, item_rows, item_tab, item_seg = [0], [], [], []
        for b, p in enumerate(plans):
            finish_sample(p, stats[b], stats[B + b], cfg, sampler, draws[b])
            base = out_offsets[-1]
            tab[b], tab[B + b] = p.tab_t, p.tab_s
            seg_tab[b] = (*p.mean, base, 1.0)
            seg_tab[B + b] = (*p.mean, base + p.n_t, 0.0)
            at = base + p.n_t + p.n_s
            for q, it in enumerate(p.items):
                item_rows.append(it.rows)
                item_tab.append(p.item_tab[q][None])
                item_seg.append((*p.mean, at, 0.0))
                at += it.n
            assert at == base + p.n_out
            out_offsets.append(at)
        m = out_offsets[-1]
        out = {"xyz_mid": torch.empty((m, 3), dtype=torch.float32, device=dev), "labels": torch.empty(m, dtype=torch.int32, device=dev),
               "mask1": torch.empty(m, dtype=torch.uint8, device=dev), "mask2": torch.empty(m, dtype=torch.uint8, device=dev)}
        _emit(xyz, labels, cub, blk_cnt, offsets, total, centre_d, tab, seg_tab, out, stream)
        for i0 in range(0, len(item_rows), _lib.MIX_MAX_SEGMENTS):                           # queue cuboids: one more launch
            rows = [r.to(dev) for r in item_rows[i0:i0 + _lib.MIX_MAX_SEGMENTS]]
            ioff = [0]
            for r in rows:
                ioff.append(ioff[-1] + r.shape[0])
            _emit(torch.cat(rows, 0).contiguous(), None, None, None, ioff, 0, None, np.stack(item_tab[i0:i0 + len(rows)]),
                  np.array(item_seg[i0:i0 + len(rows)]), out, stream)
        # tail-class cuboids of the target scenes, unmixed, for the queue
        ex_base = np.full((2 * B, total + 1), -1, dtype=np.int64)
        n_rows, wanted = 0, []
        for b, p in enumerate(plans):
            for s in sorted({s for lst in p.tail_splits for s in lst}):
                ex_base[b, s] = n_rows
                wanted.append((b, s, n_rows, int(stats[b, s, 3:].sum())))
                n_rows += wanted[-1][3]
        cuboids = {}
        if wanted:
            rows = extract(xyz, labels, cub, blk_cnt, offsets, total, centre_d, ex_base, n_rows, stream)
            roff = [w[2] for w in wanted] + [n_rows]
            rb = segment_bounds(rows, roff, stream).cpu().numpy()                            # read-back 3: the cuboids' maxima
            for k, (b, s, r0, n) in enumerate(wanted):
                hist = stats[b, s, 3:3 + K].copy()
                cuboids[(b, s)] = Cuboid(rows[r0:r0 + n], rb[k, 1], stats[b, s, :3].astype(np.float64) / FIX, hist, K)
        tail, ratio = [], None
        for b, p in enumerate(plans):
            tail.extend([[cuboids[(b, s)] for s in lst] for lst in p.tail_splits])
            ratio = p.class_ratio if ratio is None else ratio + p.class_ratio
        out["mask1"], out["mask2"] = out["mask1"].view(torch.bool), out["mask2"].view(torch.bool)
        out.update(offsets=out_offsets, tar_tail_splits=tail, tar_splits_class_ratio=ratio)
        if return_debug:
            out["debug"] = {"cub": cub, "stats": stats, "bounds": bounds, "plans": plans, "planes": planes, "centre": centre}
        return out
