"""Generates tests/golden/tacm_golden.npz in the BUILD container (needs /root/reference).

    python tests/golden/make_tacm_golden.py

The reference's own `tacm` (dataset/augmentor/augmentor_utils.py) and `SplitSampler` (dataset/augmentor/data_augmentor.py) are
imported from where they lie and run on seeded scenes; nothing of their text is copied — the file holds numbers only: per case
the recorded random draws, the queue cuboids handed out, what the run computed on the way (bounds, planes, per-cuboid
statistics, split status, kept cuboids) and its outputs.  Imports this image lacks (open3d, cv2, the reference's compiled ops)
get empty stand-ins; the loaded module sees numpy through a thin facade whose `full` casts its fill value first (numpy 2 raises
on np.full(n, 255, dtype=np.int8) where numpy 1 wrapped to -1) and whose `random` records every draw.

Every case runs twice: on its fp32 inputs and on the same inputs widened to fp64 (the reference's code is then an fp64
evaluation of itself); labels and masks of the two must agree.  Stored: the fp32 run's positions, the difference of the two,
`ref_dev` = max |fp32 run - fp64 run| and `E` = the largest |coordinate| at any stage.

tests/tacm_cases.py regenerates the inputs from the seeds (they are not stored)."""
import importlib.util
import os
import random as pyrandom
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = "/root/reference"

import tacm_cases as tc   # noqa: E402


class Recorder:
    def __init__(self):
        self.draws = []


class NpRandomFacade:
    def __init__(self, rec):
        self.rec = rec

    def rand(self, *shape):
        v = np.random.rand(*shape)
        if np.size(v) > 0:       # (np.random.rand(0, 4), the reference's empty stand-in for "no queue cuboids", draws nothing)
            self.rec.draws.append(("rand", np.array(v, dtype=np.float64)))
        return v

    def permutation(self, x):
        v = np.random.permutation(x)
        self.rec.draws.append(("permutation", np.array(v, dtype=np.float64)))
        return v

    def choice(self, a, size=None, p=None):
        v = np.random.choice(a, size, p=p)
        self.rec.draws.append(("choice", np.array(v, dtype=np.float64).reshape(-1)))
        return v


class NpFacade:
    def __init__(self, rec):
        self.random = NpRandomFacade(rec)

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def full(shape, fill_value, dtype=None, **kw):
        if dtype is not None:
            fill_value = np.array(fill_value).astype(dtype)
        return np.full(shape, fill_value, dtype=dtype, **kw)


class PyRandomFacade:
    """random.sample(population, k) -> recorded as indices; the cuboids handed out are copied as they are at that moment."""

    def __init__(self, rec):
        self.rec, self.handed = rec, []

    def sample(self, population, k):
        idx = pyrandom.sample(range(len(population)), k)
        self.rec.draws.append(("sample", np.array(idx, dtype=np.float64)))
        self.handed.extend(np.array(population[i], dtype=np.float64).copy() for i in idx)
        return [population[i] for i in idx]


def load_reference(rec):
    for name in ("open3d", "cv2", "lib", "lib.pointgroup_ops", "lib.pointgroup_ops.functions"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["lib.pointgroup_ops.functions"].pointgroup_ops = None
    spec = importlib.util.spec_from_file_location("ref_augmentor_utils", os.path.join(REF, "dataset/augmentor/augmentor_utils.py"))
    au = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(au)
    au.np = NpFacade(rec)
    # data_augmentor.py imports its sibling and the dataset package: give it the module loaded above and an empty package
    for name in ("dataset", "dataset.dataset", "dataset.augmentor"):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    sys.modules["dataset.augmentor"].augmentor_utils = au
    sys.modules["dataset.augmentor.augmentor_utils"] = au
    spec = importlib.util.spec_from_file_location("dataset.augmentor.data_augmentor", os.path.join(REF, "dataset/augmentor/data_augmentor.py"))
    da = importlib.util.module_from_spec(spec)
    da.__package__ = "dataset.augmentor"
    spec.loader.exec_module(da)
    da.np = NpFacade(rec)
    pyr = PyRandomFacade(rec)
    da.random = pyr
    return au, da, pyr


class Param(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def make_param(case):
    return Param(enabled=True, split=list(case["split"]), p=case["p"], mix_ratio=case["mix_ratio"],
                 permute_cuboid=Param(enabled=True, p=case["permute_p"]),
                 cuboid_queue=Param(enabled=case["queue"], size=case["queue_size"], num_cuboid=case["num_cuboid"],
                                    num_class=tc.NUM_CLASS, update_class_ratio=True))


def trace(au, log):
    """Wrap the module-level helpers tacm() calls so that their results are recorded."""
    orig = {k: getattr(au, k) for k in ("split_space", "get_split_idx", "tail_cuboids_from_sampler", "filter_by_index", "transform_xyz")}

    def transform_xyz(xyz, param):
        if xyz.shape[0] > 0:
            log["stage_max"] = max(log.get("stage_max", 0.0), float(np.abs(xyz).max()))
        out = orig["transform_xyz"](xyz, param)
        if out.shape[0] > 0:
            log["stage_max"] = max(log.get("stage_max", 0.0), float(np.abs(out).max()))
        return out

    def split_space(xyz, split):
        out = orig["split_space"](xyz, split)
        log.setdefault("planes", []).append((np.array(out[0], dtype=np.float64), np.array(out[1], dtype=np.float64)))
        log.setdefault("centred", []).append(np.array(xyz).copy())
        return out

    def get_split_idx(param, xyz, label, coord, rng, **args):
        out = orig["get_split_idx"](param, xyz, label, coord, rng, **args)
        log.setdefault("split_idx", []).append(np.array(out[0]).astype(np.int64).copy())
        if "calc_split" in args:
            log["split_status0"] = np.array(out[1]["split_status"]).copy()
        return out

    def tail_cuboids_from_sampler(param, n, split_status, sampler, **args):
        log["split_status"], log["n_tar"] = np.array(split_status).copy(), n
        return orig["tail_cuboids_from_sampler"](param, n, split_status, sampler, **args)

    def filter_by_index(e_list, idx):
        log.setdefault("masks", []).append(np.array(idx).copy())
        return orig["filter_by_index"](e_list, idx)

    for k, f in (("split_space", split_space), ("get_split_idx", get_split_idx),
                 ("tail_cuboids_from_sampler", tail_cuboids_from_sampler), ("filter_by_index", filter_by_index),
                 ("transform_xyz", transform_xyz)):
        setattr(au, k, f)
    return orig


def np_stats(centred, labels, split_idx, total):
    """[total + 1, 3 + K + 1] int64 as doda_mix_classify lays them out (row `total`: points of no cuboid)."""
    K = tc.N_CLASSES
    st = np.zeros((total + 1, 3 + K + 1), dtype=np.int64)
    fx = np.rint(centred.astype(np.float64) * tc.FIX).astype(np.int64)
    row = np.where(split_idx < 0, total, split_idx)
    bins = np.where((labels >= 0) & (labels < K), labels, K)
    for r in range(total + 1):
        m = row == r
        st[r, :3] = fx[m].sum(0)
        st[r, 3:] = np.bincount(bins[m], minlength=K + 1)
    return st


def run_case(au, da, pyr, rec, case, dtype):
    """One run of the reference's tacm() -> dict of what it computed."""
    t_xyz, t_lab, s_xyz, s_lab = tc.case_inputs(case)
    class_ratio = tc.class_ratio_of(t_lab)
    param = make_param(case)
    sampler = da.SplitSampler(param.cuboid_queue)
    param.cuboid_queue.class_ratio = class_ratio
    sampler.init_class_ratio(param.cuboid_queue)
    sampler.update_cfg(param.cuboid_queue)
    np.random.seed(case["seed"])
    pyrandom.seed(case["seed"])
    if case["queue"] and case["warm"]:      # fill the queue from another pair, as training would have
        w = dict(case, seed=case["seed"] + 7919, p=0.0, queue=True, num_cuboid=0.0)
        wt, wl, ws, wsl = tc.case_inputs(w)
        _, _, others = au.tacm(param, sampler, "scannet", [str(i) for i in range(tc.N_CLASSES)],
                               [wt.astype(dtype), wl.copy(), {}], [ws.astype(dtype), wsl.copy(), {}])
        sampler.update([list(x) for x in others["tar_tail_splits"]])
        assert sum(q.cur_size for q in sampler.queues) > 0
    rec.draws.clear()
    pyr.handed.clear()
    log = {}
    orig = trace(au, log)
    try:
        xyz, lab, others = au.tacm(param, sampler, "scannet", [str(i) for i in range(tc.N_CLASSES)],
                                   [t_xyz.astype(dtype), t_lab.copy(), {}], [s_xyz.astype(dtype), s_lab.copy(), {}])
    finally:
        for k, f in orig.items():
            setattr(au, k, f)
    total = int(np.prod(case["split"]))
    # the largest |coordinate| at any stage: centred, moved, shrunk, recentred
    E = max(float(np.abs(xyz).max()) if xyz.size else 0.0, max(float(np.abs(c).max()) for c in log["centred"]), log.get("stage_max", 0.0))
    return dict(xyz=np.asarray(xyz), label=np.asarray(lab).astype(np.int64), pc1_mask=np.asarray(others["pc1_mask"]),
                tail=[[np.array(a, dtype=np.float64) for a in lst] for lst in others["tar_tail_splits"]],
                ratio=np.asarray(others["tar_splits_class_ratio"], dtype=np.float64), draws=list(rec.draws), handed=list(pyr.handed),
                log=log, E=E, class_ratio=class_ratio, tail_class_idx=np.array(sampler.tail_class_idx),
                class_thres=np.array(param.cuboid_queue.class_thres), total=total,
                inputs=(t_xyz, t_lab, s_xyz, s_lab))


def sampler_record(da, rec):
    """SplitSampler / Queue against recorded values: sizes, tail classes, thresholds, ring-buffer wrap-around, three steps of
    update_class_ratio."""
    ratio = tc.SAMPLER_CLASS_RATIO
    cq = Param(enabled=True, size=tc.SAMPLER_SIZE, num_cuboid=2.0, num_class=3, update_class_ratio=True, class_ratio=ratio.copy())
    s = da.SplitSampler(cq)
    s.init_class_ratio(cq)
    s.update_cfg(cq)
    out = {"sampler_queue_sizes": np.array([q.size for q in s.queues]), "sampler_tail_class_idx": np.array(s.tail_class_idx),
           "sampler_tail_class_ratio0": np.array(s.tail_class_ratio), "sampler_inverse": np.array(s.inverse_class_ratio),
           "sampler_class_thres": np.array(cq.class_thres)}
    q = da.Queue(5)                                          # ring buffer: integers stand for cuboids
    states = []
    for batch in tc.QUEUE_UPDATES:
        q.update_queue(list(batch))
        states.append([-1 if v is None else v for v in q.queue] + [q.ptr, q.cur_size])
    out["queue_states"] = np.array(states)
    steps = []
    for r in tc.SAMPLER_RATIO_STEPS:
        s.update_class_ratio(np.array(r, dtype=np.float64))
        steps.append(np.array(s.tail_class_ratio))
    out["sampler_tail_class_ratio_steps"] = np.array(steps)
    return out


def main():
    rec = Recorder()
    au, da, pyr = load_reference(rec)
    out = dict(sampler_record(da, rec))
    cover = dict(mix_on=0, mix_off=0, perm_on=0, perm_off=0, empty_target=0, queue=0, splits=set())
    for i, case in enumerate(tc.CASES):
        a = run_case(au, da, pyr, rec, case, np.float32)
        b = run_case(au, da, pyr, rec, case, np.float64)
        assert a["xyz"].shape == b["xyz"].shape and np.array_equal(a["label"], b["label"]) and np.array_equal(a["pc1_mask"], b["pc1_mask"]), i
        assert len(a["draws"]) == len(b["draws"]) and all(x[0] == y[0] and np.array_equal(x[1], y[1]) for x, y in zip(a["draws"], b["draws"]))
        for k in range(2):
            assert np.array_equal(a["log"]["split_idx"][k], b["log"]["split_idx"][k]), (i, "cuboid ids differ between fp32 and fp64")
        dev = a["xyz"].astype(np.float64) - b["xyz"].astype(np.float64)
        ref_dev = float(np.abs(dev).max()) if dev.size else 0.0
        log, total = a["log"], a["total"]
        pre = "c%d_" % i
        kinds = [d[0] for d in a["draws"]]
        out[pre + "draw_kinds"] = np.array(kinds)
        out[pre + "draw_lens"] = np.array([-1 if d[1].ndim == 0 else d[1].size for d in a["draws"]])
        out[pre + "draw_vals"] = np.concatenate([d[1].reshape(-1) for d in a["draws"]])
        out[pre + "n_items"] = np.array(len(a["handed"]))
        for q, it in enumerate(a["handed"]):
            assert np.array_equal(it.astype(np.float32).astype(np.float64), it)
            out[pre + "item%d" % q] = it.astype(np.float32)
        # fp32 run's positions: float32 where that is exact, else float64; the fp64 run as a small difference
        x32 = a["xyz"].astype(np.float32)
        out[pre + "xyz"] = x32 if np.array_equal(x32.astype(np.float64), a["xyz"].astype(np.float64)) else a["xyz"].astype(np.float64)
        out[pre + "dev"] = dev.astype(np.float32)
        out[pre + "label"] = a["label"].astype(np.int16)
        out[pre + "n_pc1"] = np.array(int(a["pc1_mask"].sum()))
        assert a["pc1_mask"][:int(a["pc1_mask"].sum())].all()
        out[pre + "ratio"] = a["ratio"]
        out[pre + "tail_rows"] = np.array([[x.shape[0] for x in lst] + [-1] * (total - len(lst)) for lst in a["tail"]])
        out[pre + "tail_label_hist"] = np.array([[np.bincount(x[:, 3].astype(np.int64), minlength=256) for x in lst] +
                                                 [np.zeros(256, dtype=np.int64)] * (total - len(lst)) for lst in a["tail"]]).astype(np.int32)
        out[pre + "ref_dev"], out[pre + "E"] = np.array(ref_dev), np.array(a["E"])
        out[pre + "class_ratio"], out[pre + "tail_class_idx"], out[pre + "class_thres"] = a["class_ratio"], a["tail_class_idx"], a["class_thres"]
        t_xyz, t_lab, s_xyz, s_lab = a["inputs"]
        out[pre + "bounds"] = np.array([[t_xyz.min(0), t_xyz.max(0)], [s_xyz.min(0), s_xyz.max(0)]], dtype=np.float32)
        out[pre + "coord"] = np.array([log["planes"][0][0], log["planes"][1][0]])
        out[pre + "range"] = np.array([log["planes"][0][1], log["planes"][1][1]])
        out[pre + "stats"] = np.array([np_stats(log["centred"][0], t_lab, log["split_idx"][0], total),
                                       np_stats(log["centred"][1], s_lab, log["split_idx"][1], total)])
        out[pre + "split_status0"], out[pre + "split_status"] = log["split_status0"], log["split_status"]
        kept = []
        for k in range(2):
            ids, m = log["split_idx"][k], log["masks"][k]
            ids = np.where(ids < 0, total - 1, ids)
            ks = np.unique(ids[m])
            assert not np.isin(ids[~m], ks).any()          # a cuboid is kept whole or not at all
            kept.append(np.isin(np.arange(total), ks))
        out[pre + "kept"] = np.array(kept)
        out[pre + "cub_t_unassigned"] = np.array(int((log["split_idx"][0] < 0).sum()))
        # coverage
        d = a["draws"]
        mix = float(d[6][1]) < case["p"]
        perm_pos = 8 if mix else 7
        perm = float(d[perm_pos][1]) < case["permute_p"]
        cover["mix_on" if mix else "mix_off"] += 1
        cover["perm_on" if perm else "perm_off"] += 1
        cover["empty_target"] += int(a["pc1_mask"].sum() == 0)
        cover["queue"] += int(len(a["handed"]) > 0)
        cover["splits"].add(tuple(case["split"]))
        print("case %d: %d + %d -> %d points, mix %s permute %s, %d queue cuboids, ref_dev %.3g, E %.3g" % (
            i, t_xyz.shape[0], s_xyz.shape[0], a["xyz"].shape[0], mix, perm, len(a["handed"]), ref_dev, a["E"]))
    assert cover["mix_on"] and cover["mix_off"] and cover["perm_on"] and cover["perm_off"] and cover["empty_target"], cover
    assert cover["queue"] >= 2 and {(2, 2, 1), (2, 1, 2)} <= cover["splits"], cover
    out["n_cases"] = np.array(len(tc.CASES))
    path = os.path.join(HERE, "tacm_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
