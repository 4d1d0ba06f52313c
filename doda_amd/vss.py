"""Virtual scan simulation, DATA_AUG.aug_list's `vss`, on the device (reference dataset/augmentor/augmentor_utils.py:108-251,
data_augmentor.py:195-204).

  device (include/doda_vss.h)   bounds of the labelled points -> occupancy planes -> per view: range mask + count, spherical flip
                                + direction-cell keys, the hull-vertex decision per masked point -> jitter + stable compaction
  host (this file, numpy fp64)  the frame, the eroded occupancy image and the camera candidates, the per-view scalars, the window
                                of the vertex decision (window_of) — every random number from one `draws` object per sample in the
                                reference's order: rand() for p, rand() for the camera height, per attempt randint(cameras) and
                                randint(walls), rand() for random_jitter.p, rand(3 N)

The operator is the reference's: a point of a view is kept iff its flip is a vertex of the convex hull of the flipped points and
the camera.  DESIGN.md §23 derives the window bound and lists what is unpinned (open3d and cv2 are not installed here)."""
import math

import numpy as np
import torch

from . import _lib, segments
from ._lib import check, lib
from .segments import offsets_h, stream_handle

MODES = ("fixed", "parallel", "perspective")
THETA0 = 0.15            # smallest half-angle of the window of the vertex decision (radians)
THETA_MAX = 0.5          # a window wider than this is not worth its cells: the decision runs against all points
MAX_IMAGE_CELLS = 1 << 24


def _check_key(key):
    from .aug import check_key
    return check_key(key)


def _p_of(key):
    return key["p"] if isinstance(key, dict) and "p" in key else None


class VssConfig:
    """The DATA_AUG.vss section (cfgs/dataset_cfgs/front3d/front3d_cfg.yaml:50-60) with the class names and the ignore label of
    the dataset.  A missing or disabled section is a disabled configuration and is not looked at further."""

    def __init__(self, section=None, class_names=(), ignore_label=255):
        self.section = section
        self.enabled = bool(_check_key(section)) and isinstance(section, dict)
        self.class_names = [str(c) for c in (class_names or [])]
        self.ignore_label = int(ignore_label)
        if not self.enabled:
            return
        self.p = _p_of(section)
        self.value = int(section.get("value", 4))
        self.mode = str(section.get("mode", "fixed"))
        if self.mode not in MODES:
            raise ValueError("DATA_AUG.vss.mode: unknown mode %r (known: %s)" % (self.mode, ", ".join(MODES)))
        self.radius = float(section.get("radius", 1000))
        self.camera_view = float(section.get("camera_view", 180))
        self.random_jitter = section.get("random_jitter", None)
        if self.value < 1 or not self.radius > 0:
            raise ValueError("DATA_AUG.vss: value (views) and radius must be positive")
        for need in ("wall", "floor"):
            if need not in self.class_names:
                raise ValueError("DATA_AUG.vss needs the class %r among the dataset's class names (%d given)" % (need, len(self.class_names)))
        self.wall, self.floor = self.class_names.index("wall"), self.class_names.index("floor")
        self.ceiling = self.class_names.index("ceiling") if "ceiling" in self.class_names else -1


# ------------------------------------------------------------------------------------------------ the plan (host, fp64)
def window_bound(r_min, r_max, theta0=THETA0):
    """The largest |t| for which no flipped point farther than the angle theta0 from a query's direction can bind in the query's
    linear program, given r_min <= |p'| <= r_max for every flipped point: T = (r_min / r_max - cos theta0) / sin theta0 (DESIGN.md
    §23), or 0.0 where that is not positive: no window."""
    if not (r_min > 0.0 and r_max >= r_min):
        return 0.0
    t = (r_min / r_max - math.cos(theta0)) / math.sin(theta0)
    return t if t > 0.0 else 0.0


def window_of(radius, dmax):
    """(G, hinv, half, theta0) of a view whose points lie within dmax of the camera: direction cells per axis, their inverse edge
    and the half side of the box of the windowed program; G = 0: no window.  theta0 grows with the relative depth range."""
    r_max, r_min = 2.0 * radius, 2.0 * radius - dmax
    if not r_min > 0.0:
        return 0, 0.0, 0.0, 0.0
    theta0 = max(THETA0, 1.5 * math.acos(min(1.0, r_min / r_max)))
    bound = window_bound(r_min, r_max, theta0)
    if theta0 > THETA_MAX or bound <= 0.0:
        return 0, 0.0, 0.0, 0.0
    h = 2.0 * math.sin(theta0 / 2.0) * (1.0 + 1e-9)      # the chord of theta0: within theta0 = within one cell per axis
    g = int(2.0 / h) + 1
    if g > _lib.VSS_MAX_GRID:
        return 0, 0.0, 0.0, 0.0
    return g, 1.0 / h, bound / math.sqrt(2.0) * (1.0 - 1e-9), theta0


def erode(img, kh, kw):
    """cv2.erode(img, ones((kh, kw))) as its documentation states it: the minimum over the kernel anchored at (kh // 2, kw // 2),
    pixels outside the image not taking part; an empty kernel stands for the 3 x 3 one."""
    if kh < 1 or kw < 1:
        kh = kw = 3
    H, W = img.shape
    out = img.copy()
    for i in range(kh):
        for j in range(kw):
            dr, dc = i - kh // 2, j - kw // 2
            r0, r1, c0, c1 = max(0, -dr), min(H, H - dr), max(0, -dc), min(W, W - dc)
            if r0 < r1 and c0 < c1:
                out[r0:r1, c0:c1] = np.minimum(out[r0:r1, c0:c1], img[r0 + dr:r1 + dr, c0 + dc:c1 + dc])
    return out


def frame_of(lo32, hi32):
    """The frame of occlusion_simulation (:124-125) and of the occupancy image (:180-184) from the fp32 bounds of the labelled
    points: c (the subtracted point), vmin (vox_xyz_min), (H, W) of the image, the height, and the fp64 bounds of _xyz."""
    lo64, hi64 = np.asarray(lo32, dtype=np.float64), np.asarray(hi32, dtype=np.float64)
    mid = (lo64 + hi64) / 2.0                            # (fp64 like everything after it: the reference on float64 rows)
    c = np.array([mid[0], mid[1], lo64[2]])
    lo, hi = lo64 - c, hi64 - c
    vmin = lo * 10
    top = (hi * 10 - vmin).astype(np.int64)
    return c, vmin, (int(top[0]) + 3, int(top[1]) + 3), float(hi[2]), lo, hi


def candidates_of(occ, inst, vmin):
    """Camera candidates (x, y) [K, 2] from the two occupancy planes (:196-205)."""
    img = np.where((occ != 0) & (inst == 0), 255, 0).astype(np.uint8)
    H, W = img.shape
    er = erode(img, min(10, int(H / 10)), min(10, int(W / 10)))
    rr, cc = np.where(er > 0)
    cells = np.concatenate((rr.reshape(-1, 1) - 1, cc.reshape(-1, 1) - 1), 1)
    return (cells + vmin[:2]) / 10, img, er


def view_row(vcfg, c, interest, camera):
    """The 16 scalars of doda_vss_view for one (camera, interest point) pair (:216-251), fp64."""
    cam = camera - interest
    row = np.zeros(16)
    row[0:3], row[3:6], row[6:9] = c, interest, cam
    rhs = cam[0] ** 2 + cam[1] ** 2
    row[10] = rhs
    if vcfg.mode == "fixed":
        row[11], row[12] = (cam[2], -np.inf) if cam[2] > 0 else (np.inf, cam[2])
        return row
    angle = vcfg.camera_view / 180.0 * np.pi
    with np.errstate(all="ignore"):
        pitch = np.arcsin(-cam[2] / (np.linalg.norm(cam) + 10e-10))
        up, low = np.tan(pitch + angle / 2.), np.tan(pitch - angle / 2.)
        if vcfg.mode == "parallel":
            row[11], row[12] = np.sqrt(rhs) * up + cam[2], np.sqrt(rhs) * low + cam[2]
        else:
            row[9], row[13], row[14], row[15] = 1.0, np.sqrt(rhs), up, low
    return row


class _Sample:
    def __init__(self):
        self.fires = self.exit_all = False
        self.views = self.tries = self.n_wall = 0
        self.cams = np.zeros((0, 2))
        self.cam_h = 0.0
        self.wall_idx = None
        self.c = np.zeros(3)
        self.lo = self.hi = np.zeros(3)
        self.log = []                                    # (camera, interest, mask count) per attempt


# ------------------------------------------------------------------------------------------------ device calls
def decide(flipped, keys, counts, wins, selected, stream=None, exhaustive=False, stats=None):
    """The vertex decision of one round of views: flipped fp64 [N, 3] and keys int32 [N] as doda_vss_flip left them, counts[s]
    masked points and wins[s] = (G, hinv, half, key_base) per segment; ORs the decision into selected uint8 [N].
    exhaustive: every point against all points of its view (the cross-check and the fallback), no window."""
    L, st = lib(), stream_handle(stream)
    B, M = len(counts), int(sum(counts))
    if M == 0:
        return
    skeys, order = torch.sort(keys, stable=True)
    order = order[:M]
    index = order.to(torch.int32)
    pts = flipped.index_select(0, order).contiguous()
    begin = np.zeros(B + 1, dtype=np.int32)
    begin[1:] = np.cumsum(counts)
    win = np.ascontiguousarray(wins, dtype=np.float64).reshape(B, 4)
    cells = int(max(w[3] + max(1.0, w[0] ** 3) for w in win))
    cell_start = torch.searchsorted(skeys[:M].contiguous(), torch.arange(cells + 1, dtype=torch.int32, device=keys.device)).to(torch.int32)
    state = torch.zeros(M, dtype=torch.uint8, device=keys.device)
    args = (pts.data_ptr(), index.data_ptr(), begin.ctypes.data_as(_lib.c_i32p), B, cell_start.data_ptr(), win.ctypes.data_as(_lib.c_f64p))
    check(L.doda_vss_extreme(*args, None, M, _lib.VSS_EXHAUSTIVE if exhaustive else 0, selected.data_ptr(), state.data_ptr(), st),
          "doda_vss_extreme")
    undecided = 0
    if not exhaustive:
        und = torch.nonzero(state == 2).flatten().to(torch.int32)            # (read-back: the count)
        undecided = int(und.numel())
        if undecided:
            check(L.doda_vss_extreme(*args, und.data_ptr(), undecided, _lib.VSS_EXHAUSTIVE, selected.data_ptr(), state.data_ptr(), st),
                  "doda_vss_extreme")
    if stats is not None:
        windowed = int(sum(c for c, w in zip(counts, win) if w[0] > 0 and w[2] > 0 and not exhaustive))
        stats.append({"points": M, "windowed": windowed, "undecided": undecided, "kept": int((state == 1).sum())})


def hidden_point_removal(points, camera, radius, exhaustive=False, stats=None):
    """open3d's PointCloud.hidden_point_removal(camera, radius) on the device for one cloud: fp64 points [n, 3] (device) -> bool [n],
    the points that are vertices of the hull of their flips and the camera.  (The pipeline's views go through doda_vss_view /
    doda_vss_flip; this entry flips with torch and serves tests and tools.)"""
    assert points.is_cuda and points.dtype == torch.float64 and points.dim() == 2 and points.shape[1] == 3
    n = points.shape[0]
    q = points - torch.as_tensor(np.asarray(camera, dtype=np.float64), device=points.device)
    norm = q.norm(dim=1, keepdim=True)
    norm = torch.where(norm == 0, torch.full_like(norm, 0.0001), norm)
    flipped = (q + 2 * (radius - norm) * q / norm).contiguous()
    dmax = float(norm.max()) * (1.0 + 1e-9) if n else 0.0
    g, hinv, half, _ = (0, 0.0, 0.0, 0.0) if exhaustive else window_of(radius, dmax)
    keys = torch.zeros(n, dtype=torch.int32, device=points.device)
    if g > 0:
        unit = flipped / flipped.norm(dim=1, keepdim=True)
        cell = ((unit + 1.0) * hinv).to(torch.int32).clamp_(0, g - 1)
        keys = ((cell[:, 0] * g + cell[:, 1]) * g + cell[:, 2]).to(torch.int32)
    selected = torch.zeros(n, dtype=torch.uint8, device=points.device)
    decide(flipped, keys, [n], [(g, hinv, half, 0)], selected, exhaustive=exhaustive, stats=stats)
    return selected.bool()


def run(xyz, labels, offsets, vcfg, draws, masks=None, stream=None, return_debug=False, exhaustive=False):
    """The vss stage of a batch: None when it runs for no sample (disabled, or no sample's p fires), else the batch after it —
    {"xyz" fp32 [M, 3] (jittered), "labels" int32 [M], "offsets" M + 1 integers, "index" int32 [M] (the kept points' numbers),
    "masks" (compacted, or None)}.  Raises aug.EmptySample when a sample keeps no point."""
    from .aug import EmptySample
    B, n = len(offsets) - 1, int(offsets[-1])
    sizes = [int(offsets[b + 1]) - int(offsets[b]) for b in range(B)]
    S = [_Sample() for _ in range(B)]
    for b, s in enumerate(S):
        s.fires = vcfg.enabled and sizes[b] > 0 and (vcfg.p is None or bool(draws[b].rand() < vcfg.p))
    if not any(s.fires for s in S):
        return None
    if B > _lib.VSS_MAX_SEGMENTS:
        raise ValueError("vss: at most %d scenes per call" % _lib.VSS_MAX_SEGMENTS)
    dev, L, st = xyz.device, lib(), stream_handle(stream)
    arr, ns = offsets_h(offsets)
    nb = max(1, segments.n_blocks(L, "doda_vss_blocks", offsets))
    ignore = vcfg.ignore_label
    stats = [] if return_debug else None

    def up(a, dtype=np.float64):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)

    # the frame: bounds and number of the labelled points
    part, bounds_d = torch.empty((nb, 6), dtype=torch.float32, device=dev), torch.empty((B, 2, 3), dtype=torch.float32, device=dev)
    cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    check(L.doda_vss_bounds(xyz.data_ptr(), labels.data_ptr(), arr, ns, ignore, part.data_ptr(), bounds_d.data_ptr(), cnt.data_ptr(), st),
          "doda_vss_bounds")
    bounds, labelled = bounds_d.cpu().numpy(), cnt.cpu().numpy()             # read-back: 28 B per scene
    frame, dims, vmins, at = np.zeros((B, 8)), {}, {}, 0
    for b, s in enumerate(S):
        if not s.fires:
            continue
        if labelled[b] == 0:
            s.exit_all = True
            continue
        s.c, vmin, (H, W), s.height, s.lo, s.hi = frame_of(bounds[b, 0], bounds[b, 1])
        if H * W > MAX_IMAGE_CELLS:
            raise ValueError("vss: an occupancy image of %d x %d cells" % (H, W))
        frame[b] = (*s.c, vmin[0], vmin[1], H, W, at)
        dims[b], vmins[b] = (H, W, at), vmin
        at += 2 * H * W
    if at:
        img = torch.zeros(at, dtype=torch.uint8, device=dev)
        check(L.doda_vss_image(xyz.data_ptr(), labels.data_ptr(), arr, ns, ignore, vcfg.floor, vcfg.ceiling, up(frame).data_ptr(),
                               img.data_ptr(), at, st), "doda_vss_image")
        img_h = img.cpu().numpy()                                            # read-back: two bytes per 10 cm cell
    for b, s in enumerate(S):
        if b not in dims:
            continue
        H, W, base = dims[b]
        planes = img_h[base:base + 2 * H * W].reshape(2, H, W)
        s.cams, s.image, s.eroded = candidates_of(planes[0], planes[1], vmins[b])
        s.cam_h = draws[b].rand() * s.height / 2.0 + s.height / 2.0
        if s.cams.shape[0] == 0:
            s.exit_all = True
            continue
        a = int(offsets[b])
        s.wall_idx = torch.nonzero(labels[a:a + sizes[b]] == vcfg.wall).flatten() + a
        s.n_wall = int(s.wall_idx.numel())                                   # (read-back: 8 B per scene)
    # the views, in lockstep over the batch
    selected = torch.zeros(n, dtype=torch.uint8, device=dev)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    flipped, keys = torch.empty((n, 3), dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    while True:
        active = [b for b, s in enumerate(S) if s.fires and not s.exit_all and s.views < vcfg.value]
        if not active:
            break
        cams, picks = {}, {}
        for b in active:
            s = S[b]
            k = int(draws[b].randint(s.cams.shape[0]))
            cams[b] = np.array([s.cams[k, 0], s.cams[k, 1], s.cam_h])
            if s.n_wall > 0:
                picks[b] = int(draws[b].randint(s.n_wall))
        interest = {b: np.zeros(3) for b in active}
        if picks:
            order = sorted(picks)
            rows = torch.stack([S[b].wall_idx[picks[b]] for b in order])
            got = xyz.index_select(0, rows).cpu().numpy().astype(np.float64)  # read-back: 12 B per scene
            for k, b in enumerate(order):
                interest[b] = got[k] - S[b].c
        view = np.zeros((B, 16))
        view[:, 9] = -1.0
        for b in active:
            view[b] = view_row(vcfg, S[b].c, interest[b], cams[b])
        view_d = up(view)
        cnt.zero_()
        check(L.doda_vss_view(xyz.data_ptr(), labels.data_ptr(), arr, ns, ignore, view_d.data_ptr(), mask.data_ptr(), cnt.data_ptr(), st),
              "doda_vss_view")
        got = cnt.cpu().numpy()                                              # read-back: 4 B per scene
        counts, wins, grid, key_base = [0] * B, np.zeros((B, 4)), np.zeros((B, 4)), 0
        grid[:, 0] = 1.0
        for b in active:
            s = S[b]
            s.log.append((cams[b], interest[b], int(got[b])))
            if got[b] < 10:
                s.tries += 1
                if s.tries > max(5, vcfg.value):
                    s.exit_all = True
                mask[int(offsets[b]):int(offsets[b + 1])] = 0
                continue
            far = np.maximum(np.abs(s.lo - cams[b]), np.abs(s.hi - cams[b]))
            g, hinv, half, _ = (0, 0.0, 0.0, 0.0) if exhaustive else window_of(vcfg.radius, float(np.linalg.norm(far)) * (1.0 + 1e-9))
            counts[b], wins[b], grid[b] = int(got[b]), (g, hinv, half, key_base), (vcfg.radius, hinv, g, key_base)
            key_base += max(1, g ** 3)
            s.views += 1
        if sum(counts):
            check(L.doda_vss_flip(xyz.data_ptr(), arr, ns, view_d.data_ptr(), mask.data_ptr(), grid.ctypes.data_as(_lib.c_f64p),
                                  flipped.data_ptr(), keys.data_ptr(), st), "doda_vss_flip")
            decide(flipped, keys, counts, wins, selected, stream, exhaustive, stats)
    # the exits that return every labelled point, and the samples vss does not run for
    for b, s in enumerate(S):
        a, e = int(offsets[b]), int(offsets[b + 1])
        if not s.fires:
            selected[a:e] = 1
        elif s.exit_all:
            selected[a:e] = (labels[a:e] != ignore).to(torch.uint8)
    # the noise: (rand(N, 3) - 0.5) * value over ALL points of the sample, then the selection
    noise = None
    rj = vcfg.random_jitter
    for b, s in enumerate(S):
        if s.fires and _check_key(rj) and (_p_of(rj) is None or draws[b].rand() < _p_of(rj)):
            if noise is None:
                noise = np.zeros((n, 3))
            noise[int(offsets[b]):int(offsets[b + 1])] = (np.asarray(draws[b].rand(sizes[b] * 3)).reshape(sizes[b], 3) - 0.5) * rj["value"]
    noise_d = up(noise) if noise is not None else None
    cnt.zero_()
    blk_cnt = torch.empty(nb, dtype=torch.int32, device=dev)
    check(L.doda_vss_count(selected.data_ptr(), arr, ns, cnt.data_ptr(), blk_cnt.data_ptr(), st), "doda_vss_count")
    kept = cnt.cpu().numpy()                                                 # read-back: 4 B per scene
    for b in range(B):
        if kept[b] == 0:
            raise EmptySample(b)
    out_offsets = [0] + [int(v) for v in np.cumsum(kept)]
    m = out_offsets[-1]
    out_base = np.array(out_offsets[:-1], dtype=np.int64)
    out = {"xyz": torch.empty((m, 3), dtype=torch.float32, device=dev), "labels": torch.empty(m, dtype=torch.int32, device=dev),
           "index": torch.empty(m, dtype=torch.int32, device=dev), "offsets": out_offsets, "masks": None}
    om = [None, None]
    if masks is not None:
        masks = [t.view(torch.uint8) if t.dtype == torch.bool else t for t in masks]
        assert all(t.dtype == torch.uint8 and t.is_contiguous() and t.numel() == n for t in masks) and len(masks) == 2
        om = [torch.empty(m, dtype=torch.uint8, device=dev) for _ in range(2)]
        out["masks"] = om
    ptr = lambda t: t.data_ptr() if t is not None else None
    check(L.doda_vss_emit(xyz.data_ptr(), ptr(noise_d), labels.data_ptr(), ptr(masks[0]) if masks else None,
                          ptr(masks[1]) if masks else None, arr, ns, selected.data_ptr(), blk_cnt.data_ptr(),
                          out_base.ctypes.data_as(_lib.c_i64p), ptr(out["xyz"]), ptr(out["labels"]), ptr(out["index"]), ptr(om[0]), ptr(om[1]),
                          m, st), "doda_vss_emit")
    if return_debug:
        out["debug"] = {"samples": S, "selected": selected, "stats": stats}
    return out
