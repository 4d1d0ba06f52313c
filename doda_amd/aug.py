"""DATA_AUG.aug_list = [scene_aug, elastic, crop, shuffle] on the device (reference dataset/augmentor/data_augmentor.py:171-235,
dataset/augmentor/augmentor_utils.py:61-104,449-472, dataset/scannet.py:69-78).

The reference augments every sample with numpy / scipy in DataLoader workers.  Here the points stay on the device:

  device (include/doda_aug.h)   affine + bounds -> [blur -> displace + bounds] per elastic pass -> crop test + count per crop
                                iteration -> emit (stable compaction, truncation to voxel coordinates)
  host (this file, numpy fp64)  the matrix (scene_matrix), the grid shapes and the noise (grid_shape, draw_noise), the crop rule
                                (CropPlan) — every random number from one `draws` object per sample, in the reference's order:
                                jitter randn(3, 3), flip rand, rotation rand + 3 rand, elastic rand, 3 randn(bb) per pass,
                                rand(3) per crop iteration

`shuffle` is accepted and does nothing (a row permutation of the points: DESIGN.md §2).  `vss` is accepted as the FIRST entry (where
every reference config has it: it needs the untransformed scene in metres, z up) and runs before everything else (doda_amd.vss);
anywhere else it raises NotImplementedError.  Deviations from the reference are listed in DESIGN.md §13."""
import math

import numpy as np
import torch

from . import _lib, segments, vss
from ._lib import check, lib
from .segments import SeededDraws, launch_on, offsets_h, per_sample, stream_handle   # noqa: F401  (SeededDraws: for the callers)

KNOWN = ("scene_aug", "elastic", "crop", "shuffle")
MAX_REDRAWS = 4          # an emptied sample is drawn again at most this often (reference dataset/scannet.py:72-73 recurses)


class EmptySample(RuntimeError):
    """A sample of the batch kept no point (the reference's data_dict['valid'] = False)."""

    def __init__(self, index):
        super().__init__("augmentation left sample %d of the batch without points" % index)
        self.index = index


# ------------------------------------------------------------------------------------------------ configuration
def check_key(key):
    """augmentor_utils.check_key: absent = off, a bool is itself, a section is on unless `enabled: False`."""
    if key is None:
        return False
    if isinstance(key, bool):
        return key
    if isinstance(key, dict):
        return bool(key.get("enabled", True))
    return True


def _p_of(key):
    """The `p` of a section, or None where check_p would not draw."""
    return key["p"] if isinstance(key, dict) and "p" in key else None


class AugConfig:
    """The DATA_AUG section of a dataset config (cfgs/dataset_cfgs/scannet/scannet_cfg.yaml:18-32) with what DATA_PROCESSOR adds
    (voxel_scale, full_scale, max_npoint, point_range).  No DATA_AUG.aug_list, or DATA_AUG.enabled false, is a disabled one."""

    def __init__(self, aug_list=None, scene_aug=None, elastic=None, voxel_scale=50, full_scale=(128, 512), max_npoint=250000,
                 point_range=200000000, enabled=True, vss_section=None, class_names=None, ignore_label=255):
        self.aug_list = [str(a) for a in (aug_list or [])]
        self.enabled = bool(enabled) and len(self.aug_list) > 0
        for k, a in enumerate(self.aug_list):
            if a == "vss":
                if k != 0:
                    raise NotImplementedError("DATA_AUG.aug_list: vss (virtual scan simulation) must come first in the list: it "
                                              "works on the untransformed scene (metres, z up)")
                continue
            if a not in KNOWN:
                raise ValueError("DATA_AUG.aug_list: unknown entry %r (known: %s)" % (a, ", ".join(KNOWN)))
        self.scene_aug, self.elastic = scene_aug, elastic
        self.voxel_scale, self.full_scale = voxel_scale, [int(v) for v in full_scale]
        self.max_npoint, self.point_range = int(max_npoint), point_range
        self.vss_section, self.class_names, self.ignore_label = vss_section, list(class_names or []), int(ignore_label)
        # the vss stage: the section where the list names it (first), a disabled configuration otherwise
        self.vss = vss.VssConfig(vss_section if (self.enabled and "vss" in self.aug_list) else None, self.class_names, self.ignore_label)
        if self.enabled and "elastic" in self.aug_list and check_key(self.elastic):
            for gran_fac, _ in self.elastic["value"]:
                if not gran_fac * self.voxel_scale // 50 >= 1:
                    raise ValueError("DATA_AUG.elastic: granularity %s * voxel_scale // 50 is below one voxel" % gran_fac)

    @classmethod
    def from_cfg(cls, data_cfg, class_names=None):
        """From a dataset config (cfg.DATA_CONFIG or cfg.DATA_CONFIG_TAR).  class_names: the names the labels carry where a class
        mapper replaced the dataset's own (DATA_CLASS.class_names otherwise); only vss reads them."""
        proc = data_cfg.get("DATA_PROCESSOR", {}) or {}
        klass = data_cfg.get("DATA_CLASS", {}) or {}
        kw = dict(class_names=class_names or klass.get("class_names", None), ignore_label=klass.get("ignore_label", 255),
                  voxel_scale=proc.get("voxel_scale", 50), full_scale=proc.get("full_scale", [128, 512]),
                  max_npoint=proc.get("max_npoint", 250000), point_range=proc.get("point_range", 200000000))
        sec = data_cfg.get("DATA_AUG", None)
        if sec is None or "aug_list" not in sec:
            return cls(enabled=False, **kw)
        return cls(aug_list=sec["aug_list"], scene_aug=sec.get("scene_aug", None), elastic=sec.get("elastic", None),
                   enabled=sec.get("enabled", True), vss_section=sec.get("vss", None), **kw)

    def with_list(self, aug_list):
        """The same configuration under another aug_list (the cuboid-mixing dataset's [elastic, crop, shuffle],
        dataset/mix_dataset.py:18)."""
        return AugConfig(aug_list, self.scene_aug, self.elastic, self.voxel_scale, self.full_scale, self.max_npoint,
                         self.point_range, self.enabled, self.vss_section, self.class_names, self.ignore_label)


# ------------------------------------------------------------------------------------------------ randomness
class RandomStateDraws:
    """Replays numpy's legacy global stream after numpy.random.seed(seed) — the stream the reference draws from — and keeps the
    kinds and sizes of the draws asked for (`log`)."""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)
        self.log = []

    def rand(self, n=None):
        self.log.append(("rand", 1 if n is None else int(n)))
        return self.rs.rand() if n is None else self.rs.rand(n)

    def randn(self, shape):
        shape = tuple(int(v) for v in shape)
        self.log.append(("randn", int(np.prod(shape))))
        return self.rs.randn(*shape)

    def randint(self, n):
        """numpy.random.randint(n), which numpy.random.choice(n) draws too."""
        self.log.append(("randint", 1))
        return int(self.rs.randint(int(n)))


# ------------------------------------------------------------------------------------------------ the plan (host, fp64)
def scene_matrix(cfg, draws):
    """augmentor_utils.scene_aug's matrix (:87-102), or None where the step does not run (not in the list / disabled)."""
    aug = cfg.scene_aug
    if "scene_aug" not in cfg.aug_list or not check_key(aug):
        return None
    p = _p_of(aug)
    if p is not None and not draws.rand() < p:
        return None
    m = np.eye(3)
    if check_key(aug.get("jitter", None)):
        m += draws.randn((3, 3)) * 0.1
    flip = aug.get("flip", None)
    if check_key(flip) and (_p_of(flip) is None or draws.rand() < _p_of(flip)):
        m[0][0] *= -1
    rot = aug.get("rotation", None)
    if check_key(rot) and (_p_of(rot) is None or draws.rand() < _p_of(rot)):
        tx = (draws.rand() * 2 * math.pi - math.pi) * rot["value"][0]
        ty = (draws.rand() * 2 * math.pi - math.pi) * rot["value"][1]
        tz = (draws.rand() * 2 * math.pi - math.pi) * rot["value"][2]
        rx = np.array([[1, 0, 0], [0, math.cos(tx), -math.sin(tx)], [0, math.sin(tx), math.cos(tx)]])
        ry = np.array([[math.cos(ty), 0, math.sin(ty)], [0, 1, 0], [-math.sin(ty), 0, math.cos(ty)]])
        rz = np.array([[math.cos(tz), math.sin(tz), 0], [-math.sin(tz), math.cos(tz), 0], [0, 0, 1]])
        m = np.matmul(m, rx.dot(ry).dot(rz))
    return m


def elastic_fires(cfg, draws):
    """data_augmentor.elastic's check_func (:173): in the list, enabled, and its p (one draw, where it has one) fires."""
    el = cfg.elastic
    if "elastic" not in cfg.aug_list or not check_key(el):
        return False
    p = _p_of(el)
    return p is None or bool(draws.rand() < p)


def elastic_params(cfg):
    """[(gran, mag)] per pass (data_augmentor.py:175-178)."""
    return [(gran_fac * cfg.voxel_scale // 50, mag_fac * cfg.voxel_scale / 50) for gran_fac, mag_fac in cfg.elastic["value"]]


def grid_shape(lo, hi, gran):
    """bb = np.abs(x).max(0).astype(np.int32) // gran + 3 (augmentor_utils.py:66) from the exact bounds of x."""
    absmax = np.maximum(-np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64))
    if not np.all(np.isfinite(absmax)) or absmax.max() >= 2.0 ** 31:
        raise ValueError("elastic: a scene needs finite coordinates")
    return (absmax.astype(np.int32) // gran + 3).astype(np.int64)


def draw_noise(bb, draws):
    """Three randn(bb) grids cast to fp32 (augmentor_utils.py:67): fp32 [3, b0, b1, b2]."""
    return np.stack([draws.randn(bb).astype(np.float32) for _ in range(3)])


class CropPlan:
    """augmentor_utils.crop (:449-472) of one sample as a state machine around the device's counts: the volume rule, then
    next_test() per loop iteration.  lo / hi: the exact bounds of data_dict['xyz'] BEFORE the subtraction of its minimum."""

    def __init__(self, lo, hi, n, cfg):
        self.lo = np.asarray(lo, dtype=np.float64)
        # xyz.max(0) - xyz.min(0) of xyz - lo: the subtraction is monotone, the minimum is exactly 0
        self.room = (np.asarray(hi, dtype=np.float64) - self.lo) - 0.0
        self.full = np.array([cfg.full_scale[1]] * 3, dtype=np.float64)
        self.max_npoint, self.count, self.n = cfg.max_npoint, int(n), int(n)
        self.offset = np.zeros(3)
        self.tests = []                              # (offset, full_scale) of every test launched, in order
        curr = self.room[0] * self.room[1] * self.room[2]
        self.volume = bool(n > 0 and curr > cfg.point_range)
        if self.volume:
            crop_scale = math.sqrt(cfg.point_range / curr)
            self.full = np.minimum(self.full, np.array([crop_scale * self.room[0], crop_scale * self.room[1], self.room[2]]))

    def volume_test(self):
        """(offset, full_scale) of the volume rule's test (:463), or None when the rule does not fire."""
        if not self.volume:
            return None
        self.tests.append((np.zeros(3), self.full.copy()))
        return self.tests[-1]

    def next_test(self, draws):
        """(offset, full_scale) of the next loop iteration (:466-470), or None when at most max_npoint points are valid."""
        if self.count <= self.max_npoint:
            return None
        self.offset = np.clip(self.full - self.room + 0.001, None, 0) * draws.rand(3)
        self.tests.append((self.offset.copy(), self.full.copy()))
        self.full[:2] -= 32
        return self.tests[-1]

    @property
    def tested(self):
        return len(self.tests) > 0


# ------------------------------------------------------------------------------------------------ device calls
def n_blocks(offsets):
    return segments.n_blocks(lib(), "doda_aug_blocks", offsets)


def blur_grids(noise, bbs, stream=None):
    """The six box blurs on a batch's grids, in place (doda_aug_blur).  noise: fp32 device tensor, the segments' [3, b0, b1, b2]
    grids concatenated; bbs: int [n_seg, 3] (0 0 0: no grid)."""
    assert noise.is_cuda and noise.dtype == torch.float32 and noise.is_contiguous()
    bb = np.ascontiguousarray(bbs, dtype=np.int32)
    assert int(3 * bb.astype(np.int64).prod(1).sum()) == noise.numel()
    tmp = torch.empty_like(noise)
    check(lib().doda_aug_blur(noise.data_ptr(), tmp.data_ptr(), bb.ctypes.data_as(_lib.c_i32p), bb.shape[0], stream_handle(stream)),
          "doda_aug_blur")
    return noise


def _run(xyz, labels, offsets, cfg, draws, masks, stream, return_debug, batch0):
    dev, B, n = xyz.device, len(offsets) - 1, int(offsets[-1])
    L, st = lib(), stream_handle(stream)
    arr, ns = offsets_h(offsets)
    sizes = [int(offsets[b + 1]) - int(offsets[b]) for b in range(B)]
    nb = max(1, n_blocks(offsets))
    f64 = dict(dtype=torch.float64, device=dev)
    dbg = {"bounds": [], "bb": [], "grids": []} if return_debug else None

    def up(a, dtype=np.float64):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)

    # scene_aug: the matrices, then xyz_middle = xyz @ m and xyz = xyz_middle * voxel_scale
    mats = [scene_matrix(cfg, draws[b]) for b in range(B)]
    mat = np.stack([np.eye(3) if m is None else m for m in mats])
    mat_d = up(mat)
    pos, part, bounds_d = torch.empty((n, 3), **f64), torch.empty((nb, 6), **f64), torch.empty((B, 2, 3), **f64)
    check(L.doda_aug_affine(xyz.data_ptr(), arr, ns, mat_d.data_ptr(), float(cfg.voxel_scale), pos.data_ptr(), part.data_ptr(),
                            bounds_d.data_ptr(), st), "doda_aug_affine")
    bounds = bounds_d.cpu().numpy()                                          # read-back: 48 B per scene
    if dbg is not None:
        dbg["bounds"].append(bounds.copy())
    # elastic: per pass the grid shapes from the bounds, the noise from the host's stream, blur + displace on the device
    fires = [elastic_fires(cfg, draws[b]) and sizes[b] > 0 for b in range(B)]
    feat_scale = 0.0
    if any(fires):
        if bool(cfg.elastic.get("apply_to_feat", False)):
            if not all(fires[b] or sizes[b] == 0 for b in range(B)):
                raise NotImplementedError("elastic.apply_to_feat with p < 1: xyz_middle would differ per sample of a batch")
            feat_scale = float(cfg.voxel_scale)
        for gran, mag in elastic_params(cfg):
            bbs, gm, grids = np.zeros((B, 3), dtype=np.int32), np.zeros((B, 2)), []
            for b in range(B):
                if fires[b]:
                    bb = grid_shape(bounds[b, 0], bounds[b, 1], gran)
                    if int(bb.prod()) > _lib.AUG_MAX_GRID_CELLS:
                        raise ValueError("elastic: a noise grid of %s cells" % (tuple(int(v) for v in bb),))
                    bbs[b], gm[b] = bb, (gran, mag)
                    grids.append(draw_noise(bb, draws[b]).reshape(-1))
            noise = blur_grids(up(np.concatenate(grids), np.float32), bbs, stream)
            check(L.doda_aug_displace(pos.data_ptr(), arr, ns, noise.data_ptr(), bbs.ctypes.data_as(_lib.c_i32p),
                                      gm.ctypes.data_as(_lib.c_f64p), part.data_ptr(), bounds_d.data_ptr(), st), "doda_aug_displace")
            new = bounds_d.cpu().numpy()                                     # read-back: 48 B per scene
            for b in range(B):
                if fires[b]:
                    bounds[b] = new[b]
            if dbg is not None:
                dbg["bounds"].append(bounds.copy())
                dbg["bb"].append(bbs.copy())
                dbg["grids"].append(noise)
    # crop: the volume rule, then one test per loop iteration while a scene holds more than max_npoint valid points
    do_crop = "crop" in cfg.aug_list
    plans = [CropPlan(bounds[b, 0], bounds[b, 1], sizes[b], cfg) for b in range(B)]
    valid = blk_cnt = None
    if do_crop:
        rnd = 0
        while True:
            tests = [p.volume_test() if rnd == 0 else p.next_test(draws[b]) for b, p in enumerate(plans)]
            if rnd == 0 and all(t is None for t in tests):
                rnd = 1
                continue
            if all(t is None for t in tests):
                break
            if valid is None:
                valid = torch.empty(n, dtype=torch.uint8, device=dev)
                blk_cnt = torch.empty(nb, dtype=torch.int32, device=dev)
            par = np.zeros((B, 10))
            for b, t in enumerate(tests):
                if t is not None:
                    par[b, 0:3], par[b, 3:6], par[b, 6:9] = plans[b].lo, t[0], t[1]
                    par[b, 9] = 2.0 if len(plans[b].tests) == 1 else 1.0
            count = torch.zeros(B, dtype=torch.int32, device=dev)
            check(L.doda_aug_crop(pos.data_ptr(), arr, ns, up(par).data_ptr(), valid.data_ptr(), count.data_ptr(),
                                  blk_cnt.data_ptr(), st), "doda_aug_crop")
            got = count.cpu().numpy()                                        # read-back: 4 B per scene
            for b, t in enumerate(tests):
                if t is not None:
                    plans[b].count = int(got[b])
            rnd += 1
    for b, p in enumerate(plans):
        if p.count == 0:
            raise EmptySample(b)
    # emit: the kept points in their order
    out_offsets = [0]
    for p in plans:
        out_offsets.append(out_offsets[-1] + p.count)
    m = out_offsets[-1]
    par = np.zeros((B, 10))
    for b, p in enumerate(plans):
        par[b, 0:3], par[b, 3:6] = p.lo, p.offset
    seg_valid = np.array([1 if p.tested else 0 for p in plans], dtype=np.int32)
    out_base = np.array(out_offsets[:-1], dtype=np.int64)
    out = {"locs32": torch.empty((m, 4), dtype=torch.int32, device=dev), "locs_float": torch.empty((m, 3), dtype=torch.float32, device=dev),
           "labels32": torch.empty(m, dtype=torch.int32, device=dev)}
    om = [None, None]
    if masks is not None:
        masks = [t.view(torch.uint8) if t.dtype == torch.bool else t for t in masks]
        assert all(t.dtype == torch.uint8 and t.is_contiguous() and t.numel() == n for t in masks) and len(masks) == 2
        om = [torch.empty(m, dtype=torch.uint8, device=dev) for _ in range(2)]
    top = torch.zeros(3, dtype=torch.int32, device=dev)
    any_valid = bool(seg_valid.any())
    ptr = lambda t: t.data_ptr() if t is not None else None
    check(L.doda_aug_emit(xyz.data_ptr(), pos.data_ptr(), labels.data_ptr(), ptr(masks[0]) if masks else None,
                          ptr(masks[1]) if masks else None, arr, ns, mat_d.data_ptr(), feat_scale, up(par).data_ptr(),
                          ptr(valid) if any_valid else None, ptr(blk_cnt) if any_valid else None,
                          seg_valid.ctypes.data_as(_lib.c_i32p), out_base.ctypes.data_as(_lib.c_i64p), int(batch0), ptr(out["locs32"]),
                          ptr(out["locs_float"]), ptr(out["labels32"]), ptr(om[0]), ptr(om[1]), top.data_ptr(), m, st), "doda_aug_emit")
    if any_valid:
        top_h = top.cpu().numpy().astype(np.int64)                           # read-back: 12 B
    else:       # nothing dropped: the largest coordinate is trunc(max - min) (the subtraction and the truncation are monotone)
        top_h = np.max([(p.room).astype(np.int64) + 1 for p in plans if p.n > 0], 0)
    out["offsets"] = torch.tensor(out_offsets, dtype=torch.int32)
    out["spatial_shape"] = np.clip(top_h, cfg.full_scale[0], None)
    if masks is not None:
        out["mask1"], out["mask2"] = om[0].view(torch.bool), om[1].view(torch.bool)
    if dbg is not None:
        dbg.update(pos=pos, mat=mat, plans=plans, valid=valid if any_valid else None, fires=fires, top=top)
        out["debug"] = dbg
    return out


@torch.no_grad()
def augment_batch(xyz_mid, labels, offsets, cfg, draws, masks=None, stream=None, return_debug=False, batch0=0):
    """Augment a batch of scenes under cfg.aug_list (the reference's DataAugmentor.forward per sample, then what its collate_fn
    makes of the samples).

    xyz_mid fp32 [N, 3] (metres), labels int32 [N], offsets B + 1 host integers; draws: one draws object per sample (or one
    object, for a batch of one) — rand(), rand(n), randn(shape), consumed in the reference's order; masks: None or two uint8 /
    bool tensors [N] that are compacted with the points; `stream`: the stream to launch on (default: torch's current stream; the
    small read-backs block the calling thread only — the loader thread).
    -> the dictionary DeviceScenes._finish returns without "id": locs32 int32 [M, 4] (batch index batch0 + b, voxel
    coordinates), locs_float fp32 [M, 3], labels32 int32 [M], offsets int32 [B + 1], spatial_shape; plus mask1 / mask2 when masks
    were given.  Raises EmptySample when a sample keeps no point.  With `vss` first in the list the virtual scans run first
    (doda_amd.vss.run: occlusion + jitter, compacted) and the rest of the list sees their output."""
    if not cfg.enabled:
        raise ValueError("augment_batch: the configuration has no DATA_AUG.aug_list")
    B = len(offsets) - 1
    if B > _lib.AUG_MAX_SEGMENTS:
        raise ValueError("augment_batch: at most %d scenes per call" % _lib.AUG_MAX_SEGMENTS)
    draws = per_sample(draws, B, "augment_batch")
    assert xyz_mid.is_cuda and xyz_mid.dtype == torch.float32 and xyz_mid.dim() == 2 and xyz_mid.shape[1] == 3
    assert int(offsets[-1]) == xyz_mid.shape[0] == labels.shape[0]
    xyz_mid, labels, offsets = xyz_mid.contiguous(), labels.to(torch.int32).contiguous(), [int(v) for v in offsets]
    with launch_on(stream):
        scan = vss.run(xyz_mid, labels, offsets, cfg.vss, draws, masks, stream, return_debug) if cfg.vss.enabled else None
        if scan is not None:     # the rest of the list sees the scanned, jittered samples
            xyz_mid, labels, offsets, masks = scan["xyz"], scan["labels"], scan["offsets"], scan["masks"]
        out = _run(xyz_mid, labels, offsets, cfg, draws, masks, stream, return_debug, batch0)
        if return_debug:
            out["debug"]["vss"] = scan
        return out
