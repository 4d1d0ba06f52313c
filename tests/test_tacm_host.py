"""Tail-aware cuboid mixing, host side (no GPU): the companion C ABI include/doda_mix.h, the mixing plan and the split sampler of
doda_amd.tacm against what the reference's own tacm() / SplitSampler computed (tests/golden/tacm_golden.npz, made by
tests/golden/make_tacm_golden.py), the new config and the command line."""
import numpy as np
import pytest

from tests import tacm_cases as tc


def test_mix_entry_points_report_bad_arguments(native_lib):
    """Argument errors come back as statuses without a launch: offsets that do not start at 0 or decrease, too many segments,
    cuboids or classes, null pointers; an empty batch is nothing to do."""
    import ctypes as C
    lib = native_lib
    off = lambda *v: (C.c_int64 * len(v))(*v)
    assert lib.doda_mix_blocks(off(0, 1024, 1025, 1025), 3) == 2
    assert lib.doda_mix_blocks(off(1, 5), 1) == -1 and lib.doda_mix_blocks(off(0, 5, 4), 2) == -1
    assert lib.doda_mix_blocks(off(0, 1 << 31), 1) == -1
    assert lib.doda_mix_bounds(1, 3, off(0, 5, 4), 2, 1, 1, None) == -1                    # decreasing offsets
    assert lib.doda_mix_bounds(1, 5, off(0, 5), 1, 1, 1, None) == -4                       # stride 5
    assert lib.doda_mix_bounds(None, 3, off(0, 5), 1, 1, 1, None) == -1                    # no points
    assert lib.doda_mix_bounds(1, 3, off(*range(130)), 129, 1, 1, None) == -4              # 129 segments
    assert lib.doda_mix_classify(1, 1, off(0, 5), 1, 1, 1, 33, 20, 1, 1, 1, None) == -4    # 33 cuboids
    assert lib.doda_mix_classify(1, 1, off(0, 5), 1, 1, 1, 4, 33, 1, 1, 1, None) == -4     # 33 classes
    assert lib.doda_mix_classify(1, None, off(0, 5), 1, 1, 1, 4, 20, 1, 1, 1, None) == -1  # no labels
    assert lib.doda_mix_classify(None, None, off(0, 0), 1, None, None, 4, 20, None, None, None, None) == 0   # empty
    assert lib.doda_mix_emit(1, 3, 1, 1, None, off(0, 5), 1, 4, 1, 1, 1, 1, 1, 1, 1, 5, None) == -1     # cuboid ids without counts
    assert lib.doda_mix_emit(1, 3, None, None, None, off(0, 5), 1, 0, None, 1, 1, 1, 1, 1, 1, 5, None) == -1   # labels from a 3-float row
    assert lib.doda_mix_emit(1, 3, 1, 1, 1, off(0, 5), 1, 4, 1, 1, 1, 1, 1, 1, 1, -1, None) == -1      # negative output length
    assert lib.doda_mix_extract(1, 1, 1, 1, off(0, 5), 1, 0, 1, 1, 1, 5, None) == -4                  # no cuboids
    assert lib.doda_mix_extract(1, 1, 1, 1, off(0, 5), 1, 4, 1, None, 1, 5, None) == -1               # no table


# ------------------------------------------------------------------------------------------------ the plan against the reference
class GoldenSampler:
    """Stands for the reference's filled queue: hands out the cuboids the golden run was handed, consuming the recorded draws
    the way SplitSampler.get_split does (one `choice`, then one `sample` per class whose queue was not empty)."""

    def __init__(self, items, n_classes=tc.N_CLASSES):
        from doda_amd import tacm
        import torch
        self.items = [tacm.Cuboid(torch.from_numpy(np.ascontiguousarray(it)), n_classes=n_classes) for it in items]
        self.at = 0

    def get_split(self, n, draws):
        out = []
        for _ in draws.choice(tc.NUM_CLASS, n, None):
            if draws.pos < len(draws.record) and draws.record[draws.pos][0] == "sample":
                draws.sample(1, 1 << 30)
                out.append(self.items[self.at])
                self.at += 1
        return out


def golden_cfg(case, g):
    from doda_amd import tacm
    cfg = tacm.TacmConfig(enabled=True, split=case["split"], p=case["p"], mix_ratio=case["mix_ratio"], permute_p=case["permute_p"],
                          queue_enabled=case["queue"], queue_size=case["queue_size"], num_cuboid=case["num_cuboid"],
                          num_class=tc.NUM_CLASS, n_classes=tc.N_CLASSES)
    cfg.class_ratio, cfg.class_thres, cfg.tail_class_idx = g["class_ratio"], g["class_thres"], g["tail_class_idx"]
    return cfg


@pytest.mark.parametrize("i", range(len(tc.CASES)))
def test_plan_reproduces_the_reference_exactly(i):
    """plan() on the golden's recorded bounds, per-cuboid statistics and draws: the planes (fp64, bit for bit), the split status
    before and after the permutation, the kept cuboids of both scenes, the output size and tar_splits_class_ratio."""
    from doda_amd import tacm
    with np.load(tc.GOLDEN) as z:
        assert int(z["n_cases"]) == len(tc.CASES)
        g = tc.load_case(z, i)
    case = tc.CASES[i]
    cfg = golden_cfg(case, g)
    draws = tacm.ReplayDraws(g["draws"])
    seen = {}

    def stats(planes_t, planes_s):
        seen["planes"] = (planes_t, planes_s)
        return g["stats"][0], g["stats"][1]
    p = tacm.plan(g["bounds"], stats, cfg, GoldenSampler(g["items"]), draws)
    assert draws.exhausted()
    assert np.array_equal(p.coord_t, g["coord"][0]) and np.array_equal(p.coord_s, g["coord"][1])        # fp64 equality
    assert np.array_equal(p.range_t, g["range"][0]) and np.array_equal(p.range_s, g["range"][1])
    assert np.array_equal(seen["planes"][0][:, 1], g["coord"][0] - g["range"][0])
    assert np.array_equal(p.split_status0, g["split_status0"]) and np.array_equal(p.split_status, g["split_status"])
    total = cfg.total_splits
    assert np.array_equal(np.isin(np.arange(total), p.kept_t), g["kept"][0]) and np.array_equal(np.isin(np.arange(total), p.kept_s), g["kept"][1])
    assert np.array_equal(p.tab_t[:total, 0] != 0, g["kept"][0]) and np.array_equal(p.tab_s[:total, 0] != 0, g["kept"][1])
    assert len(p.items) == int(g["n_items"]) and p.n_out == g["label"].shape[0] and p.n_t == int(g["n_pc1"])
    assert np.array_equal(np.asarray(p.class_ratio, dtype=np.float64), g["ratio"])
    assert [len(lst) for lst in p.tail_splits] == [int((r >= 0).sum()) for r in g["tail_rows"]]
    for lst, rows in zip(p.tail_splits, g["tail_rows"]):
        assert [int(g["stats"][0][s, 3:].sum()) for s in lst] == [int(r) for r in rows[rows >= 0]]
    # the draw sequence the plan asked for, by kind: three per split_space call, check_p, ...
    kinds = [k for k, _ in g["draws"]]
    assert kinds[:7] == ["rand"] * 7
    # the sample's mean from the per-cuboid sums equals the mean of the golden's positions before the last subtraction: the fp64
    # run is centred to ~1e-16, so the plan's mean must make the golden's output mean vanish
    if p.n_out:
        out64 = g["xyz"].astype(np.float64) - g["dev"].astype(np.float64)
        assert np.abs(out64.mean(0)).max() < 1e-9


def test_golden_covers_what_the_issue_asks():
    with np.load(tc.GOLDEN) as z:
        gs = [tc.load_case(z, i) for i in range(len(tc.CASES))]
    mix = [float(g["draws"][6][1]) < c["p"] for g, c in zip(gs, tc.CASES)]
    perm = [float(g["draws"][8 if m else 7][1]) < c["permute_p"] for g, c, m in zip(gs, tc.CASES, mix)]
    assert any(mix) and not all(mix) and any(perm) and not all(perm)
    assert any(int(g["n_pc1"]) == 0 for g in gs)
    assert sum(int(g["n_items"]) > 0 for g in gs) >= 2
    assert {(2, 2, 1), (2, 1, 2)} <= {tuple(c["split"]) for c in tc.CASES}
    for g in gs:
        assert 0 < float(g["ref_dev"]) < 16 * 2.0 ** -24 * float(g["E"])


# ------------------------------------------------------------------------------------------------ the sampler
def _sampler(num_class=3):
    from doda_amd import tacm
    cfg = tacm.TacmConfig(enabled=True, queue_size=tc.SAMPLER_SIZE, num_class=num_class, n_classes=tc.N_CLASSES)
    s = tacm.SplitSampler(cfg)
    s.init_class_ratio(tc.SAMPLER_CLASS_RATIO.copy())
    s.update_cfg(cfg)
    return s, cfg


def test_split_sampler_matches_the_reference_class():
    from doda_amd import tacm
    with np.load(tc.GOLDEN) as z:
        g = {k: z[k] for k in z.files if k.startswith("sampler_") or k == "queue_states"}
    s, cfg = _sampler()
    with pytest.raises(ValueError):
        tacm.SplitSampler(cfg).get_split(1, None)                       # not initialised
    assert [q.size for q in s.queues] == list(g["sampler_queue_sizes"])
    assert np.array_equal(s.tail_class_idx, g["sampler_tail_class_idx"]) and np.array_equal(cfg.tail_class_idx, g["sampler_tail_class_idx"])
    assert np.array_equal(s.tail_class_ratio, g["sampler_tail_class_ratio0"]) and np.array_equal(s.inverse_class_ratio, g["sampler_inverse"])
    assert np.array_equal(cfg.class_thres, g["sampler_class_thres"])
    q = tacm.Queue(5)
    for batch, want in zip(tc.QUEUE_UPDATES, g["queue_states"]):
        q.update_queue(list(batch))
        assert [-1 if v is None else v for v in q.queue] + [q.ptr, q.cur_size] == list(want)
    for r, want in zip(tc.SAMPLER_RATIO_STEPS, g["sampler_tail_class_ratio_steps"]):
        s.update_class_ratio(np.array(r))
        assert np.array_equal(s.tail_class_ratio, want)


def test_split_sampler_save_load_round_trip(tmp_path):
    import torch
    from doda_amd import tacm
    s, cfg = _sampler()
    rng = np.random.default_rng(0)
    mk = lambda n: tacm.Cuboid(torch.from_numpy(np.concatenate((rng.random((n, 3)), rng.integers(0, 20, (n, 1))), 1).astype(np.float32)))
    s.update([[mk(5), mk(7)], [], [mk(3)]])
    s.update_class_ratio(np.array([1.0, 2.0, 0.0]))
    path = tmp_path / "split_sampler.pth"
    s.save_sampler(path)
    buf = torch.load(path, weights_only=False)
    assert set(buf) == {"queues", "class_ratio", "inverse_class_ratio", "tail_class_ratio", "tail_class_idx"}
    assert all(r is None or (torch.is_tensor(r) and not r.is_cuda) for q in buf["queues"] for r in q["queue"])
    t, _ = _sampler()
    t.load_sampler(path)
    assert np.array_equal(t.tail_class_ratio, s.tail_class_ratio) and np.array_equal(t.tail_class_idx, s.tail_class_idx)
    for a, b in zip(s.queues, t.queues):
        assert (a.size, a.ptr, a.cur_size, a.got) == (b.size, b.ptr, b.cur_size, b.got)
        for x, y in zip(a.queue, b.queue):
            assert (x is None) == (y is None)
            if x is not None:
                assert torch.equal(x.rows, y.rows) and np.array_equal(x.max, y.max) and np.array_equal(x.hist, y.hist) and np.array_equal(x.sum, y.sum)
    draws = tacm.ReplayDraws([("choice", np.array([0, 1, 2])), ("sample", np.array([1])), ("sample", np.array([0]))])
    got = t.get_split(3, draws)                                          # class 1's queue is empty: no draw, no cuboid
    assert draws.exhausted() and [c.n for c in got] == [7, 3]


# ------------------------------------------------------------------------------------------------ configuration and command line
def test_tacm_config_yaml_and_absent_section():
    from doda_amd import st, tacm
    _, cfg = st.parse_config(["--cfg_file", "doda_amd/cfgs/synthetic/spconv_st_tacm.yaml"])
    t = tacm.TacmConfig.from_cfg(cfg)
    assert t.enabled and t.split == [2, 2, 1] and t.p == 0.5 and t.mix_ratio == 0.5 and t.permute_enabled and t.permute_p == 0.5
    assert t.queue_enabled and t.queue_size == 256 and t.num_cuboid == 2.0 and t.num_class == 2 and t.update_class_ratio
    assert t.n_classes == 20 and t.total_splits == 4
    _, plain = st.parse_config(["--cfg_file", "doda_amd/cfgs/synthetic/spconv_st.yaml"])
    assert not tacm.TacmConfig.from_cfg(plain).enabled
    for k in ("SELF_TRAIN", "MODEL", "OPTIMIZATION", "EVALUATION", "COMMON_CLASSES", "DATA_CONFIG"):      # = spconv_st.yaml + the section
        assert cfg[k] == plain[k], k
    with pytest.raises(ValueError):
        tacm.TacmConfig(enabled=True, split=[4, 3, 3])                   # 36 cuboids
    with pytest.raises(ValueError):
        tacm.mix_batch(None, None, [0], None, None, [0], tacm.TacmConfig.from_cfg(plain), None, [])


@pytest.mark.parametrize("flag", ["--host_loader", "--inline_loader"])
def test_st_with_tacm_refuses_the_host_loaders(flag):
    """Cuboid mixing is device-only: the worker-process and the inline loader stop with a clear error before anything runs."""
    from doda_amd import st
    with pytest.raises(ValueError, match="tacm"):
        st.main(["--cfg_file", "doda_amd/cfgs/synthetic/spconv_st_tacm.yaml", flag])
