"""Scenes for the virtual-scan tests and a numpy / scipy restatement of the reference's steps (dataset/augmentor/augmentor_utils.py:
108-251), written from their semantics: the hull step is scipy.spatial.ConvexHull (qhull) on the fp64 flipped points plus the
origin, the erosion is scipy.ndimage.minimum_filter (the window of an even size k reaches from -k // 2 to k - 1 - k // 2, cv2's
default anchor), and every random number comes from one numpy RandomState in the reference's order."""
import numpy as np

CLASS_NAMES = ["wall", "floor", "cabinet", "bed", "chair", "sofa", "table", "door", "window", "bookshelf", "desk"]
WALL, FLOOR, BOX, IGNORE = 0, 1, 2, 255
CAMERAS = ((3.3, 0.7, 1.9), (2.0, 0.9, 1.4))
# the reference's 3D-FRONT values (cfgs/dataset_cfgs/front3d/front3d_cfg.yaml:34-60)
VSS = {"enabled": True, "value": 4, "mode": "fixed", "p": 1.0, "radius": 1000, "camera_view": 180,
       "random_jitter": {"enabled": True, "value": 0.01, "p": 1.0}}
DATA_AUG = {"enabled": True, "aug_list": ["vss", "scene_aug", "elastic", "crop", "shuffle"],
            "scene_aug": {"flip": {"p": 0.5}, "rotation": {"p": 1.0, "value": [0.0, 0.0, 1.0]}, "jitter": True},
            "elastic": {"enabled": True, "value": [[6, 40], [20, 160]], "apply_to_feat": False, "p": 1.0}, "shuffle": True, "vss": VSS,
            "tacm": {"enabled": False}}
PROCESSOR = {"point_range": 200000000, "voxel_scale": 50, "cache": False, "max_npoint": 250000, "full_scale": [128, 512], "voxel_mode": 4,
             "downsampling_scale": 1}


def data_cfg(vss=None, aug_list=None, class_names=CLASS_NAMES):
    sec = dict(DATA_AUG, vss=dict(VSS, **(vss or {})))
    if aug_list is not None:
        sec["aug_list"] = list(aug_list)
    return {"DATA_AUG": sec, "DATA_PROCESSOR": dict(PROCESSOR), "DATA_CLASS": {"class_names": list(class_names), "ignore_label": IGNORE}}


def _lattice(a, b, step):
    return np.arange(int(round((b - a) / step)) + 1) * step + a


def room(step=0.05, seed=7, jitter=0.005):
    """A 4 x 3 x 2.6 m room — floor, the walls x = 0 and y = 0, a 1 x 0.6 x 0.8 m box — on a lattice, every coordinate jittered
    by +-jitter: fp64 [n, 3] and labels (13 896 points at 5 cm, 3 616 at 10 cm)."""
    parts, labs = [], []

    def add(x, y, z, lab):
        g = np.stack(np.meshgrid(x, y, z, indexing="ij"), -1).reshape(-1, 3)
        parts.append(g)
        labs.append(np.full(g.shape[0], lab, dtype=np.int64))
    X, Y, Z = _lattice(0, 4, step), _lattice(0, 3, step), _lattice(0, 2.6, step)
    add(X, Y, [0.0], FLOOR)
    add([0.0], Y, Z, WALL)
    add(X, [0.0], Z, WALL)
    bx, by, bz = _lattice(1.5, 2.5, step), _lattice(1.2, 1.8, step), _lattice(0, 0.8, step)
    add(bx, by, [0.8], BOX)
    add([1.5], by, bz, BOX)
    add([2.5], by, bz, BOX)
    add(bx, [1.2], bz, BOX)
    add(bx, [1.8], bz, BOX)
    pts = np.concatenate(parts)
    rng = np.random.default_rng(seed)
    return pts + (rng.random(pts.shape) * 2 - 1) * jitter, np.concatenate(labs)


def shell(n, seed):
    """n points in general position: random directions over a half space at 1 to 4 m."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d[:, 2] = np.abs(d[:, 2])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * (1.0 + 3.0 * rng.random((n, 1)))


# ------------------------------------------------------------------------------------------------ the restatement
def flip(points, camera, radius):
    q = np.asarray(points, dtype=np.float64) - np.asarray(camera, dtype=np.float64)
    norm = np.linalg.norm(q, axis=1, keepdims=True)
    norm = np.where(norm == 0, 0.0001, norm)
    return q + 2 * (radius - norm) * q / norm


def hull_vertices(flipped):
    """bool [n]: the flipped points that qhull reports as vertices of the hull of the points and the origin."""
    from scipy.spatial import ConvexHull
    n = flipped.shape[0]
    v = ConvexHull(np.concatenate((flipped, np.zeros((1, 3))), 0)).vertices
    out = np.zeros(n, dtype=bool)
    out[v[v < n]] = True
    return out


def hidden_point_removal(points, camera, radius):
    return hull_vertices(flip(points, camera, radius))


def borderline(flipped, trials=2, rel=1e-9, seed=11):
    """bool [n]: the points whose qhull answer changes when every flipped coordinate is perturbed by a relative `rel`."""
    base = hull_vertices(flipped)
    rng = np.random.default_rng(seed)
    out = np.zeros(flipped.shape[0], dtype=bool)
    for _ in range(trials):
        out |= hull_vertices(flipped * (1.0 + rel * (rng.random(flipped.shape) * 2 - 1))) != base
    return out


def erode(img, kh, kw):
    import scipy.ndimage
    if kh < 1 or kw < 1:
        kh = kw = 3
    return scipy.ndimage.minimum_filter(img, size=(kh, kw), mode="constant", cval=255)


def camera_candidates(_xyz, labels_sel, class_names):
    """get_camera_candidate_locations without its random height: (camera xy [K, 2], image, eroded image, height)."""
    vox = _xyz * 10
    vmin = vox.min(0)
    cell = (vox - vmin).astype(np.int64)
    inst = labels_sel != class_names.index("floor")
    if "ceiling" in class_names:
        inst &= labels_sel != class_names.index("ceiling")
    img = np.zeros(cell.max(0)[:2] + 3, dtype=np.uint8)
    img[cell[:, 0] + 1, cell[:, 1] + 1] = 255
    img[cell[inst, 0] + 1, cell[inst, 1] + 1] = 0
    er = erode(img, min(10, int(img.shape[0] / 10)), min(10, int(img.shape[1] / 10)))
    rr, cc = np.where(er > 0)
    cams = (np.stack((rr - 1, cc - 1), 1) + vmin[:2]) / 10
    return cams, img, er, _xyz[:, 2].max()


def view_mask(_xyz_f, cam, mode, camera_view=180):
    front = _xyz_f[:, 0] * cam[0] + _xyz_f[:, 1] * cam[1] <= (cam[0] ** 2 + cam[1] ** 2)
    if mode == "fixed":
        return front & (_xyz_f[:, 2] < cam[2]) if cam[2] > 0 else front & (_xyz_f[:, 2] > cam[2])
    angle = camera_view / 180.0 * np.pi
    pitch = np.arcsin(-cam[2] / (np.linalg.norm(cam) + 10e-10))
    cxy = np.sqrt(cam[0] ** 2 + cam[1] ** 2)
    if mode == "parallel":
        zu, zl = cxy * np.tan(pitch + angle / 2.) + cam[2], cxy * np.tan(pitch - angle / 2.) + cam[2]
    else:
        along = (_xyz_f[:, 0] * cam[0] + _xyz_f[:, 1] * cam[1]) / cxy
        zu, zl = (cxy - along) * np.tan(pitch + angle / 2.) + cam[2], (cxy - along) * np.tan(pitch - angle / 2.) + cam[2]
    return front & (_xyz_f[:, 2] < zu) & (_xyz_f[:, 2] > zl)


def frame(xyz32, sel):
    """_xyz of occlusion_simulation (:124-125) on the fp32 points widened to float64 (the reference computes in the dtype of its
    rows; the project defines the operator on float64 rows that hold the fp32 values)."""
    pts = xyz32[sel].astype(np.float64)
    c = (pts.min(0) + pts.max(0)) / 2.0
    c = np.array([c[0], c[1], pts.min(0)[2]])
    return pts - c, c


def virtual_scan(param, xyz32, labels, class_names, rs, ignore=IGNORE):
    """virtual_scan_simulation on fp32 xyz with the RandomState `rs` -> (jittered fp32 xyz, selected bool [n], log of attempts)."""
    n = xyz32.shape[0]
    sel = labels != ignore
    log = []

    def occlusion():
        if sel.sum() == 0:
            return sel
        idx = np.arange(n)[sel]
        _xyz, _ = frame(xyz32, sel)
        cams, _, _, height = camera_candidates(_xyz, labels[sel], class_names)
        cam_h = rs.rand() * height / 2.0 + height / 2.0
        if cams.shape[0] == 0:
            return sel
        wall = _xyz[labels[sel] == class_names.index("wall")]
        out = np.zeros(n, dtype=bool)
        views = tries = 0
        while views < param["value"]:
            k = rs.randint(cams.shape[0])
            camera = np.array([cams[k, 0], cams[k, 1], cam_h])
            interest = wall[rs.choice(wall.shape[0])] if wall.shape[0] > 0 else np.zeros(3)
            cam_f, f = camera - interest, _xyz - interest
            m = view_mask(f, cam_f, param["mode"], param["camera_view"])
            log.append((camera, interest, int(m.sum())))
            if m.sum() < 10:
                tries += 1
                if tries > max(5, param["value"]):
                    return sel
                continue
            out[idx[m][hidden_point_removal(f[m], cam_f, param["radius"])]] = True
            views += 1
        return out
    selected = occlusion()
    xyz = xyz32.astype(np.float64)
    rj = param.get("random_jitter", None)
    if rj is not None and rj.get("enabled", True) and ("p" not in rj or rs.rand() < rj["p"]):
        xyz += (rs.rand(n, 3) - 0.5) * rj["value"]
    return xyz.astype(np.float32), selected, log
