"""tools/headnumerics.py on the CPU: the probe table of tests/test_gpu_head_numerics.py reaches every compiled kernel of head.hip,
lovasz.hip and loss.hip (tests/data/head_instantiations.json, regenerated from the built objects when they are there) and nothing
else, stands on both sides of every threshold of their launchers (the constants are parsed from the sources), keeps the voxels whose
argmax is undecided and the Lovasz items with a tied key below 1e-3 of every probe — and its bounds do their work: the fp64 reference
rounded once and the kernels' expressions in numpy float32 pass them, seventeen subtly wrong results (applied to the reference's own
outputs) do not, and the Lovasz near-tie slack is shown to be needed where it is used.  The Lovasz reference itself is held to doda_amd.lovasz.lovasz_softmax in fp64 and its autograd."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


hn = _load("headnumerics")
K = hn.K
PROBES = hn.probes()
GOOD = [p for p in PROBES if not p["status"]]


def find(group, **kw):
    got = [p for p in GOOD if p["group"] == group and all(p[k] == v for k, v in kw.items())]
    assert got, (group, kw)
    return got


def test_one_set_of_names():
    """Probed = compiled: 62 kernels (34 of head.hip, 23 of lovasz.hip, 5 of loss.hip)."""
    compiled = json.load(open(hn.INSTANTIATIONS))
    objs = [os.path.join(ROOT, "doda_amd", "csrc", "_obj", f) for f in hn.OBJECTS]
    if all(os.path.exists(o) for o in objs) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        assert _load("gatherroutes").instantiations(objs, hn.STEMS) == compiled
    probed = {n for p in PROBES for n in hn.kernels(p)}
    assert probed == set(compiled) and len(compiled) == 62, sorted(probed ^ set(compiled))
    head = sum(n.startswith(("head_", "st_voxel_conf")) for n in compiled)
    assert (head, sum(n.startswith("lovasz_") for n in compiled), sum(n.startswith(("ce_", "seg_meters")) for n in compiled)) == (34, 23, 5)
    assert all(not hn.kernels(p) for p in PROBES if p["status"]) and len({p["id"] for p in PROBES}) == len(PROBES)


def test_every_threshold_has_a_probe_on_each_side():
    assert (K["HD_BLOCK"], K["BUCKETS"], K["FINAL_THREADS"], K["DW_CAP"]) == (256, [12, 16, 20, 32], 1024, 1024)      # (what the issue's shapes assume)
    assert (K["LV_WTILE"], K["LV_STILE"], K["LV_BATCH"], K["SCAN_LANES"], K["SCAN_TILE"] * K["SCAN_BLOCK"]) == (4096, 2048, 4, 64, 524288)
    assert (K["CE_BLOCK"], K["CE_FWD_CAP"], K["CE_BWD_CAP"], K["METER_CAP"], K["LOVASZ_MAX_POINTS"]) == (256, 2048, 8192, 1024, 65535)
    for esz in (4, 2):
        for m in (1, K["HD_BLOCK"] - 1, K["HD_BLOCK"], K["HD_BLOCK"] + 1):
            for k in (1, 2, 32):
                find("A", esz=esz, m=m, n_cls=k)
        for e in K["BUCKETS"][:-1]:      # both sides of every bucket edge, in the head, the confidence and (one side at least) Lovasz
            assert hn.bucket(e) == e and hn.bucket(e + 1) > e
            for m in (1, 255, 256, 257):
                find("A", esz=esz, n_cls=e, m=m), find("A", esz=esz, n_cls=e + 1, m=m)
            for c in (16, 32):
                find("C", esz=esz, c=c, n_cls=e), find("C", esz=esz, c=c, n_cls=e + 1)
            find("A", esz=esz, n_cls=e + 1, bias=0)
        find("A", esz=esz, n_cls=2, bias=0)
        assert {hn.bucket(p["n_cls"]) for p in find("F", esz=esz)} == set(K["BUCKETS"])
        # head_ce_final's second turn: 1024 and 1025 partial rows
        rows = K["FINAL_THREADS"]
        assert hn.hd_blocks(find("A", esz=esz, m=rows * 256)[0]["m"]) == rows and hn.hd_blocks(find("A", esz=esz, m=rows * 256 + 1)[0]["m"]) == rows + 1
        for what, st in (("k33", hn.ERR_UNSUPPORTED), ("c32", hn.ERR_UNSUPPORTED), ("nblocks", hn.ERR_WORKSPACE)):
            assert [p for p in PROBES if p["group"] == "A" and p["esz"] == esz and p["what"] == what and p["status"] == st]
        for fam in hn.FAMILIES:
            find("A", esz=esz, family=fam), find("C", esz=esz, family=fam)
        for ign in hn.IGNORES:
            find("A", esz=esz, ignore=ign), find("F", esz=esz, ignore=ign)
        for lists in hn.LISTS:
            find("A", esz=esz, lists=lists)
        find("A", esz=esz, grad=0.0), find("A", esz=esz, labels="allign")
        # Lovasz: the 64-item chunk, the 256-item batch, the scan and the sort tile (two items per voxel), the two second rounds
        for items in (64, 64 * K["LV_BATCH"], K["LV_STILE"], K["LV_WTILE"]):
            find("F", esz=esz, m=items // 2, n_cls=11), find("F", esz=esz, m=items // 2 + 1, n_cls=11)
        plans = [hn.lv_plan(p["m"], p["n_cls"]) for p in find("F", esz=esz)]
        assert sorted({P["stiles"] > K["SCAN_LANES"] for P in plans}) == [False, True] and max(P["stiles"] for P in plans) == K["SCAN_LANES"] + 1
        assert sorted({P["scan_tiles"] > K["SCAN_BLOCK"] for P in plans}) == [False, True]
        assert hn.lv_plan(32769, 32)["hist_len"] == 557056 > K["SCAN_TILE"] * K["SCAN_BLOCK"]
        w16 = find("F", esz=esz, lists="w16")[0]
        cnt, hist = hn.counts_hist(w16, hn.make_inputs(w16))
        assert hist[0, 1] == cnt[0] == K["LOVASZ_MAX_POINTS"] == 0xffff
        assert [p for p in PROBES if p["group"] == "F" and p["esz"] == esz and p["what"] == "ld" and p["status"] == hn.ERR_UNSUPPORTED
                and hn.make_inputs(p)["v2p"].shape[1] - 1 == K["LOVASZ_MAX_POINTS"] + 1]
        find("F", esz=esz, family="identical", m=5000), find("F", esz=esz, labels="absent"), find("F", esz=esz, bias=0)
    # head_dw_bf16: the chunk and workgroup edges, the grid cap and its grid-stride loop with a partial last chunk
    cap = K["DW_CAP"] * 256
    for m in (1, 63, 64, 65, 255, 256, 257):
        for k in (1, 2, 11, 20, 31, 32):
            find("B", m=m, n_cls=k)
    assert hn.dw_blocks(cap) == hn.dw_blocks(cap + 1) == K["DW_CAP"] and hn.dw_blocks(cap - 256) == K["DW_CAP"] - 1
    find("B", m=cap), find("B", m=cap + 1)
    assert hn.div_up(cap + 1, 64) == 4 * K["DW_CAP"] + 1      # (a second chunk for wave 0 of workgroup 0, with 63 empty lanes)
    assert len([p for p in PROBES if p["group"] == "B" and p["status"] == hn.ERR_INVALID]) == 2
    # the matrix cross-entropy: both grid caps; the meters' cap
    n = K["CE_FWD_CAP"] * K["CE_BLOCK"] * K["CE_ROWS"]
    find("D", m=n, c=5), find("D", m=n + 1, c=5)
    assert hn.ce_blocks(n) == hn.ce_blocks(n + 1) == K["CE_FWD_CAP"] and hn.div_up(n + 1, 1024) == K["CE_FWD_CAP"] + 1
    assert hn.div_up(n * 5, 1024) > K["CE_BWD_CAP"] == hn.ce_bwd_blocks(n, 5) and hn.ce_bwd_blocks(70001, 64) < K["CE_BWD_CAP"]
    for c in (1, 2, 5, 20, 63, 64):
        for m in (1, 1023, 1025, 70001):
            find("D", c=c, m=m)
    assert [p for p in PROBES if p["group"] == "D" and p["c"] == K["CE_MAX_C"] + 1 and p["status"] == hn.ERR_UNSUPPORTED]
    n = K["METER_CAP"] * 1024
    for k in (1, 20, 255, 256):
        for p64 in (0, 1):
            for p2v in (0, 1):
                find("E", n_cls=k, m=1, p64=p64, p2v=p2v), find("E", n_cls=k, m=n, p64=p64, p2v=p2v), find("E", n_cls=k, m=n + 1, p64=p64, p2v=p2v)
    assert hn.meter_blocks(n) == hn.meter_blocks(n + 1) == K["METER_CAP"] and hn.div_up(n + 1, 1024) == K["METER_CAP"] + 1
    assert [p for p in PROBES if p["group"] == "E" and p["n_cls"] == K["SM_MAX_K"] + 1 and p["status"] == hn.ERR_UNSUPPORTED]


@pytest.mark.parametrize("group", ["A", "C", "F"])
def test_leave_out_caps(group):
    """From the fp64 logits alone: undecided argmax voxels and Lovasz items with a tied fp32 key are at most 1e-3 of every probe; the
    exact family decides every voxel and holds the designed ties; the identical-voxel probes keep the bg and the fg run apart."""
    for p in [p for p in GOOD if p["group"] == group]:
        I = hn.make_inputs(p)
        _, z, Sz = hn.head_logits(p, I)
        pred = hn.pred_ref(z, Sz, p["c"], p["family"] == "exact")
        assert 1.0 - pred["decided"].mean() <= hn.MAX_LEFT_OUT, p["id"]
        k = p["n_cls"]
        if p["family"] == "exact":
            for lo, hi in ((0, k - 1), (1, 2), (3, 4)):
                if lo < hi < k and (lo, hi) not in ((0, 2), (0, 4)):      # (at three and five classes a later copy replaces the first)
                    assert np.array_equal(z[:, lo], z[:, hi]) and not (pred["top1"] == hi).any(), p["id"]
            assert p["m"] < 255 or k < 5 or (pred["top1"] == 3).any() or (pred["top1"] == 1).any() or (pred["top1"] == 0).any()
        if group == "F":
            R = hn.reference(p, I)
            assert hn.left_out(p, R)[1] <= hn.MAX_LEFT_OUT, (p["id"], hn.left_out(p, R))
            if p["family"] == "identical":
                prob = hn.softmax64(z)[0][0]
                assert (np.abs(2 * prob - 1) > 1e-3).all()


@pytest.mark.parametrize("group", hn.GROUPS)
def test_references_pass_their_own_bounds(group):
    n = 0
    for p in [p for p in GOOD if p["group"] == group and p["m"] <= hn.HOST_ROWS]:
        I = hn.make_inputs(p)
        R = hn.reference(p, I)
        for what, got in (("rounded once", hn.round_once(p, R)), ("float32", hn.emulate(p, I))):
            table, fails = hn.check(p, R, got)
            assert not fails, (p["id"], what, fails)
            n += len(table)
    assert n or group == "E"


def test_lovasz_reference_is_lovasz_softmax():
    """The weighted-item reference = the point-level definition (doda_amd.lovasz.lovasz_softmax, fp64) and its autograd."""
    from doda_amd.lovasz import lovasz_softmax
    for p in find("F", esz=4, m=129) + find("F", esz=4, m=300) + find("F", esz=4, lists="w16") + find("F", esz=4, m=1024):
        I = hn.make_inputs(p)
        R = hn.reference(p, I)
        W, z, _ = hn.head_logits(p, I)
        zv = torch.from_numpy(z).requires_grad_()
        lab = torch.from_numpy(I["labels"])
        loss = lovasz_softmax(zv[torch.from_numpy(I["pv"])], lab, p["ignore"])
        (loss * p["grad"]).backward()
        assert abs(float(loss.detach()) - R["vals"]["out0"][0]) <= 1e-12, p["id"]
        scale = np.abs(R["vals"]["dz"][0]).max()
        assert np.abs(zv.grad.numpy() - R["vals"]["dz"][0]).max() <= 1e-9 * scale, p["id"]


def _first(group, pick, **kw):
    return next(p for p in find(group, **kw) if pick(p))


plain = lambda p: p["labels"] in ("mixed", "sparse") and p["grad"] != 0 and p["bias"]
MISTAKES = [
    ("tie_high", lambda: _first("A", plain, family="exact", n_cls=5, m=300)),
    ("pad_zero", lambda: _first("A", lambda p: plain(p) and p["m"] > 1 and p["family"] == "general", n_cls=13)),
    ("mean_all", lambda: _first("A", plain, m=257, lists="ragged")),
    ("cnt_ignored", lambda: _first("A", plain, m=257, lists="ragged")),
    ("label_mod", lambda: _first("A", lambda p: plain(p) and p["n_cls"] >= 12, m=257, lists="ragged")),
    ("drop_last_odd", lambda: _first("A", lambda p: plain(p) and p["m"] >= 255, n_cls=17)),
    ("drop_last_db", lambda: _first("A", plain, m=300)),
    ("drop_rows_1024", lambda: _first("A", plain, m=K["FINAL_THREADS"] * 256 + 1, esz=4)),
    ("no_bf16_w", lambda: _first("A", lambda p: plain(p) and p["m"] >= 255 and p["n_cls"] >= 12, esz=2, family="general")),
    ("missing_chunk", lambda: _first("B", lambda p: True, m=257, n_cls=20)),
    ("stale_lanes", lambda: _first("B", lambda p: True, m=K["DW_CAP"] * 256 + 1, n_cls=11)),
    ("no_max", lambda: _first("D", lambda p: plain(p) and p["m"] >= 1023 and p["c"] >= 5, family="saturated")),
    ("swap_one", lambda: _first("F", lambda p: p["grad"] != 0 and p["mode"] == "items", m=1025)),
    ("absent_in_mean", lambda: _first("F", lambda p: p["m"] > 100, labels="absent")),
    ("carry64", lambda: _first("F", lambda p: True, m=65537, esz=4)),
    ("w15", lambda: _first("F", lambda p: True, lists="w16", esz=4)),
    ("no_clamp", lambda: _first("E", lambda p: True, n_cls=20, m=K["METER_CAP"] * 1024 + 1, p64=0, p2v=1)),
]


@pytest.mark.parametrize("wrong", [w for w, _ in MISTAKES])
def test_subtly_wrong_results_fail(wrong):
    p = dict(MISTAKES)[wrong]()
    I = hn.make_inputs(p)
    R = hn.reference(p, I)
    assert not hn.check(p, R, hn.round_once(p, R))[1]
    table, fails = hn.check(p, R, hn.round_once(p, hn.reference(p, I, wrong)))
    assert fails, (wrong, p["id"], table)
    print(wrong, p["id"], fails[:3])


def test_the_changed_lovasz_rules_are_needed():
    """Where the tool departs from a plain reading of the per-item rule, the plain form fails a correct result.  The float32
    restatement orders items by its own float32 probabilities, as the device does: on the 65 537-voxel probe it passes with the
    near-tie slack and fails gitem, dz and d_feats without it — while its summed gradients pass without any slack.  The same probe with
    the label set of the others leaves more than 1e-3 of its items tied; the saturated probe ties most of its keys."""
    p = find("F", esz=4, m=65537)[0]
    I = hn.make_inputs(p)
    got = hn.emulate(p, I)
    table, fails = hn.check(p, hn.reference(p, I), got)
    assert not fails, fails
    table, fails = hn.check(p, hn.reference(p, I, "no_slack"), got)
    failed = {f.split(":")[0] for f in fails}
    assert {"gitem", "dz", "d_feats"} <= failed and not failed & {"out0", "gsum", "dbp", "db"}, fails
    q = dict(p, labels="mixed")
    Iq = hn.make_inputs(q)
    assert hn.left_out(q, hn.reference(q, Iq))[1] > hn.MAX_LEFT_OUT >= hn.left_out(p, hn.reference(p, I))[1]
    s = find("F", esz=4, family="saturated")[0]
    Is = hn.make_inputs(s)
    assert hn.reference(s, Is)["tied"].mean() > 100 * hn.MAX_LEFT_OUT
