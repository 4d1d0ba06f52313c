#!/usr/bin/env python
"""Route probes of doda_spconv_gather_ex: one call on each side of every threshold of the kernel selection (gather_plan.hpp).

  python tools/gatherroutes.py --run main|f32split [--max-rows N]
      makes every call of the group once and prints one JSON line per call: name, status, statistics rows, SHA-256 of y and of
      the statistics rows; for the error probes whether y and the workspace kept their sentinel.  With DODA_TRACE_GATHER=1 the
      library's trace lines (route= grid= block= parts=) appear on stderr in the same order.  The group f32split expects
      DODA_F32_SPLIT_ROWS=0 in the environment.
  python tools/gatherroutes.py --numerics GROUP
      one call per reachable kernel instantiation of the group (tools/gathernumerics.py: the list is generated from the plan,
      tests/data/gather_numerics.json) against the fp64 reference: per call one JSON line with the traced route, the shape, the
      errors of y, of each statistics sum and of the prologue's side output, and whether every guard kept its sentinel.  Meant
      for a fresh process; sets DODA_TRACE_GATHER=1 (and DODA_F32_SPLIT_ROWS=0 for the group f32split) itself.
  python tools/gatherroutes.py --families
      one call per kernel family at a small shape: the largest error against the fp64 reference, one JSON line per call.
  python tools/gatherroutes.py --instantiations doda_amd/csrc/_obj/spconv_gather.o .../spconv_tile.o .../spconv_wlds.o
      the conv_* kernel symbols of the gfx950 code objects: regenerates tests/data/gather_instantiations.json.
  python tools/gatherroutes.py --instantiations --stem wgrad_multi_kernel doda_amd/csrc/_obj/spconv_wgrad.o
      the same reader for the kernels whose name starts with another stem: regenerates tests/data/wgrad_instantiations.json.
  python tools/gatherroutes.py --instantiations --stem bn_,lay_ doda_amd/csrc/_obj/bn.o doda_amd/csrc/_obj/layers.o
      several stems, separated by commas: the BatchNorm kernels, tests/data/bn_instantiations.json (tools/bnnumerics.py).
  python tools/gatherroutes.py --fold TRACE.csv RESULTS.jsonl
      joins a rocprofv3 --kernel-trace CSV of such a run with its result lines: per call the normalised conv kernel with grid and
      workgroup size and those of the pack kernel, as JSON (the form of tests/data/gather_routes.json).
Tile routes use tables and tilebooks of a raster-ordered plane of voxels (ops.rulebook_subm / ops.tilebook_build); every other
probe a random table with entries in [-1, n_in)."""
import csv
import ctypes as C
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPT = {"tile": 1, "wlds": 2, "pipeline": 4, "dual": 5, "up": 6}
SCENES = {"t12": (64, 48), "t768": (512, 384), "t769": (443, 444)}   # plane sizes: 3 072 rows, 768 tiles, 769 tiles (196 692 rows)


def probe(name, **kw):
    p = dict(name=name, esz=2, K=27, kc=16, nc=16, rows=0, n_in=None, out32=0, stats=0, scene=None, off=(), x_off=0, y_ld=0,
             packed=0, ws_short=0, res_bcast=0, pre=0, side_off=0, tb_rows=None, err=0)
    p.update(kw)
    return p


def probes(group):
    ps = []
    if group == "f32split":
        ps += [probe("s0.f32.16x16.wf%d" % wf, esz=4, rows=16 * wf) for wf in (1024, 4096)]
        ps += [probe("s0.f32.32x32.wf8192", esz=4, kc=32, nc=32, rows=16 * 8192),
               probe("s0.f32.pre1", esz=4, rows=16 * 2048, pre=1)]
        return ps
    ps += [probe("generic.f32.kc3", esz=4, kc=3, rows=1000), probe("generic.f32.xoff4", esz=4, rows=1000, x_off=4)]
    for tag, esz, kc, nc, wfs in (("bf16.16x16", 2, 16, 16, (1024, 1025, 4095, 4096)), ("f32.16x16", 4, 16, 16, (1024, 1025, 4095, 4096)),
                                  ("bf16.32x32", 2, 32, 32, (512, 513, 2047, 2048, 8191, 8192)),
                                  ("f32.32x32", 4, 32, 32, (2047, 2048, 8191, 8192)), ("bf16.64x64", 2, 64, 64, (256, 257)),
                                  ("bf16.32x48", 2, 32, 48, (511, 512, 8191, 8192)),
                                  ("bf16.32x64", 2, 32, 64, (511, 512, 2047, 2048, 8191, 8192)),
                                  ("bf16.32x96", 2, 32, 96, (255, 256, 1023, 1024, 4095, 4096))):
        ps += [probe("%s.wf%d" % (tag, wf), esz=esz, kc=kc, nc=nc, rows=16 * wf) for wf in wfs]
    ps += [probe("k1.bf16.16x16.wf1024", K=1, rows=16 * 1024), probe("k1.bf16.32x32.wf512", K=1, kc=32, nc=32, rows=16 * 512),
           probe("k1.f32.16x16.wf1024", K=1, esz=4, rows=16 * 1024), probe("k1.bf16.64x64.wf256", K=1, kc=64, nc=64, rows=16 * 256)]
    for nc in (16, 32):
        for tag, off in (("", ()), (".off", ("up",))):     # conv_up32, and the same calls with DODA_OPT_CONV_UP off
            up = lambda name, **kw: probe("up.%d.%s%s" % (nc, name, tag), K=8, kc=32, nc=nc, rows=2048, n_in=512, off=off, **kw)
            ps += [up("plain"), up("stats", stats=1), up("out32", out32=1)]
    ps += [probe("up.32.k1", K=1, kc=32, nc=32, rows=2048, n_in=512),
           probe("up.32.coarse", K=8, kc=32, nc=32, rows=2048, n_in=2048)]
    for sc in ("t768", "t769"):
        t = lambda name, **kw: probe("%s.%s" % (sc, name), scene=sc, **kw)
        ps += [t("16x16"), t("16x16.stats", stats=1), t("16x16.out32", out32=1), t("16x32.stats", nc=32, stats=1), t("16x48.stats", nc=48, stats=1)]
        for nc in (32, 64):
            for st in (0, 1):
                ps += [t("32x%d.s%d" % (nc, st), kc=32, nc=nc, stats=st), t("32x%d.s%d.nodual" % (nc, st), kc=32, nc=nc, stats=st, off=("dual",))]
        ps += [t("32x16", kc=32), t("f32.16x16", esz=4), t("16x16.nopipe", off=("pipeline",)), t("16x16.notile", off=("tile",)),
               t("16x16.rows", tb_rows=-1)]
    ps += [probe("t12.32x32.stats", scene="t12", kc=32, nc=32, stats=1), probe("t12.16x16", scene="t12")]
    ps += [probe("wlds.%d" % r, kc=48, nc=48, rows=r) for r in (8191, 8192, 262144, 262145)]
    ps += [probe("wlds.8192.stats", kc=48, nc=48, rows=8192, stats=1), probe("wlds.8192.out32", kc=48, nc=48, rows=8192, out32=1),
           probe("wlds.8192.off", kc=48, nc=48, rows=8192, off=("wlds",))]
    for kind in (1, 2, 3):
        for wf in (2048, 2049):
            ps += [probe("pre%d.bf16.32x16.wf%d" % (kind, wf), kc=32, rows=16 * wf, pre=kind),
                   probe("pre%d.f32.16x16.wf%d" % (kind, wf), esz=4, rows=16 * wf, pre=kind)]
    # error returns (last: the parent of the route plan enqueued the pack kernel before some of them)
    ps += [probe("err.pre.kc264", kc=264, rows=64, pre=1, err=-4), probe("err.pre.side", kc=32, rows=64, pre=1, side_off=4, err=-4),
           probe("err.pre.bf16.16", rows=64, pre=1, err=-4), probe("err.ystride.kc6", kc=6, rows=64, y_ld=20, err=-4),
           probe("err.packed.wide", kc=32, rows=64, x_off=8, packed=1, err=-4), probe("err.ws.short", rows=64, ws_short=1, err=-5),
           probe("err.bcast.generic", esz=4, kc=3, rows=64, res_bcast=1, err=-4)]
    return ps


def ws_short_bytes(p):
    """One byte less than the packing of the probe's own (fast-path) call needs: gather_plan.hpp pack_geometry."""
    K, kc, NB, esz = p["K"], p["kc"], (p["nc"] + 15) // 16, p["esz"]
    if esz == 2 and kc == 16 and K >= 2:        # pair
        return K * NB * 32 * 16 - 1
    if esz == 2 and kc >= 32 and kc % 8 == 0:   # wide
        return K * ((kc + 31) // 32) * NB * 64 * 16 - 1
    return K * ((kc + 15) // 16) * NB * 64 * 4 * esz - 1


def plan_line(p, group="main"):
    """The probe as a line of tests/host/gather_plan_main.cpp (the facts run() below hands to the library)."""
    rows = SCENES[p["scene"]][0] * SCENES[p["scene"]][1] if p["scene"] else p["rows"]
    kv = dict(K=p["K"], kc=p["kc"], nc=p["nc"], esz=p["esz"], n_out=rows, n_in=rows if p["scene"] else (p["n_in"] or rows),
              out32=p["out32"], stats=p["stats"], x_al=p["x_off"], y_ld=p["y_ld"], packed=p["packed"],
              res_bcast=p["res_bcast"], pre_kind=p["pre"], side=int(not p["side_off"]))
    if p["scene"]:
        kv.update(tilebook=1, tilebook_rows=rows + (p["tb_rows"] or 0))
    if p["ws_short"]:
        kv["ws_bytes"] = ws_short_bytes(p)
    for o in p["off"]:
        kv["sw." + {"pipeline": "tile_pipeline", "dual": "tile_dual", "up": "conv_up"}.get(o, o)] = 0
    if group == "f32split":
        kv["sw.f32_split_rows"] = 0
    return " ".join("%s=%d" % it for it in kv.items())


class _Prologue(C.Structure):
    _fields_ = [("kind", C.c_int32), ("relu", C.c_int32), ("rows", C.c_int32), ("c_a", C.c_int32), ("totals", C.c_void_p),
                ("totals_b", C.c_void_p), ("eps", C.c_float), ("momentum", C.c_float), ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("running_mean", C.c_void_p), ("running_var", C.c_void_p), ("num_batches_tracked", C.c_void_p), ("mean", C.c_void_p),
                ("invstd", C.c_void_p), ("side", C.c_void_p), ("side_ld", C.c_int32), ("aux_ld", C.c_int32), ("add_ld", C.c_int32),
                ("accumulate", C.c_int32), ("aux", C.c_void_p), ("add", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p)]


SENTINEL = 0x5a


def _sha(t):
    return hashlib.sha256(t.contiguous().view(-1).view(__import__("torch").uint8).cpu().numpy().tobytes()).hexdigest()[:16]


def run(group, max_rows):
    import torch
    from doda_amd import ops
    from doda_amd._lib import lib
    d = torch.device("cuda:0")
    L = lib()
    scenes = {}

    def scene(tag):
        if tag not in scenes:
            a, b = SCENES[tag]
            i, j = torch.meshgrid(torch.arange(a), torch.arange(b), indexing="ij")
            idx = torch.stack([torch.zeros(a * b, dtype=torch.long), i.reshape(-1) + 1, j.reshape(-1) + 1, torch.full((a * b,), 2)], 1)
            tbl = ops.rulebook_subm(idx.int().to(d), [a + 2, b + 2, 4], 1, 3)
            scenes[tag] = (tbl, ops.tilebook_build(tbl))
        return scenes[tag]

    for k, p in enumerate(probes(group)):
        if p["scene"]:
            tbl, tb = scene(p["scene"])
            n_out = n_in = tbl.shape[1]
        else:
            n_out, tb = p["rows"], None
            n_in = p["n_in"] or n_out
        if n_out > max_rows:
            continue
        g = torch.Generator(device="cpu").manual_seed(1000 + k)
        K, kc, nc, esz = p["K"], p["kc"], p["nc"], p["esz"]
        if not p["scene"]:
            tbl = torch.randint(-1, n_in, (K, n_out), generator=g, dtype=torch.int32).to(d)
        dt = torch.float32 if esz == 4 else torch.bfloat16
        pad = 16 // esz
        xbuf = torch.randn(n_in * kc + pad, generator=g).to(d).to(dt)
        x = xbuf[p["x_off"] // esz:]
        w = (torch.randn(K, kc, nc, generator=g) * 0.1).bfloat16().float().to(d)
        ydt = torch.float32 if (esz == 4 or p["out32"]) else torch.bfloat16
        y_ld = p["y_ld"] or nc
        y = torch.full((n_out, y_ld), 0, dtype=ydt, device=d)
        if p["err"]:
            y.view(torch.uint8).fill_(SENTINEL)
        need = L.doda_spconv_gather_workspace_bytes(K, kc, nc, esz)
        ws = torch.full((need,), SENTINEL, dtype=torch.uint8, device=d)
        ws_n = need
        if p["ws_short"]:
            ws_n = ws_short_bytes(p)
        ep = ops._ConvEpilogue()
        keep = []
        rows = C.c_int32(-1)
        stats = None
        if p["stats"]:
            stats = torch.zeros((int(L.doda_spconv_stats_capacity(n_out)), 2, nc), dtype=torch.float32, device=d)
            ep.stats, ep.stats_rows_h = stats.data_ptr(), C.pointer(rows)
        if p["res_bcast"]:
            res = torch.randn(nc, generator=g).to(d).to(ydt)
            keep.append(res)
            ep.residual, ep.residual_bcast = res.data_ptr(), 1
        if tb is not None:
            ep.tilebook, ep.tilebook_rows = tb.data_ptr(), n_out + (p["tb_rows"] or 0)
        if p["y_ld"]:
            ep.y_ld = p["y_ld"]
        if p["pre"]:
            q = _Prologue()
            f32 = lambda n, v=0.0: torch.full((n,), v, dtype=torch.float32, device=d)
            tot = torch.zeros(8 * 2 * 16 * (kc // 4), dtype=torch.float64, device=d)
            side = torch.zeros(n_in * kc + pad, dtype=dt, device=d)
            aux = torch.randn(n_in * kc, generator=g).to(d).to(dt)
            add = torch.randn(n_in * kc, generator=g).to(d).to(dt)
            vec = [f32(kc, 1.0), f32(kc, 0.25), f32(kc, 0.1), f32(kc, 1.5), f32(kc), f32(kc)]
            keep += [tot, side, aux, add, vec, q]
            q.kind, q.relu, q.rows, q.totals, q.eps, q.momentum = p["pre"], 1, n_in, tot.data_ptr(), 1e-4, 0.1
            q.gamma, q.beta, q.mean, q.invstd, q.dgamma, q.dbeta = (v.data_ptr() for v in vec)
            q.side, q.side_ld = side.data_ptr() + p["side_off"], kc
            q.aux, q.add, q.aux_ld, q.add_ld = aux.data_ptr(), add.data_ptr(), kc, kc
            ep.prologue = C.addressof(q)
        layout = 0
        w_ptr = w.data_ptr()
        if p["packed"]:
            layout, w_ptr = 0x100, ws.data_ptr()
        for o in p["off"]:
            L.doda_set_option(OPT[o], 0)
        st = L.doda_spconv_gather_ex(x.data_ptr(), n_in, kc, esz, w_ptr, nc, tbl.data_ptr(), tbl.shape[1], K, n_out, y.data_ptr(),
                                     int(bool(p["out32"])), layout, None if p["packed"] else ws.data_ptr(), ws_n, C.byref(ep), None)
        for o in p["off"]:
            L.doda_set_option(OPT[o], 1)
        torch.cuda.synchronize()
        out = {"name": p["name"], "status": st, "rows": rows.value}
        if p["err"]:
            out["y_kept"] = bool((y.view(torch.uint8) == SENTINEL).all().item())
            out["ws_kept"] = bool((ws == SENTINEL).all().item())
        else:
            out["y"] = _sha(y)
            if stats is not None:
                out["stats"] = _sha(stats[:max(rows.value, 0)])
        print(json.dumps(out), flush=True)
        del keep


# family, esz, K, kc, nc, rows (or scene), n_in: one call per kernel family at a small shape that reaches it
FAMILIES = [("conv_gather", 4, 27, 3, 16, 1000, None), ("conv_fast<PBF16P, 1, 1, 3, false, true", 2, 27, 16, 16, 4096, None),
            ("conv_fast<PBF16W, 3, 2, 3, false, true", 2, 27, 32, 48, 8192, None), ("conv_wlds48", 2, 27, 48, 48, 8192, None),
            ("conv_up32", 2, 8, 32, 32, 2048, 512), ("conv_tile<1,", 2, 27, 32, 32, "t12", None), ("conv_tile16", 2, 27, 16, 16, "t769", None)]


def families():
    """ops.spconv_gather once per FAMILIES row (bf16 rows also with fp32 output): per call one JSON line with the largest error
    against the fp64 reference, relative to the largest value; the trace lines on stderr say which kernel ran."""
    import torch
    from doda_amd import ops
    d = torch.device("cuda:0")
    for family, esz, K, kc, nc, rows, n_in in FAMILIES:
        g = torch.Generator().manual_seed(kc * 100 + nc)
        if isinstance(rows, str):
            a, b = SCENES[rows]
            i, j = torch.meshgrid(torch.arange(a), torch.arange(b), indexing="ij")
            idx = torch.stack([torch.zeros(a * b, dtype=torch.long), i.reshape(-1) + 1, j.reshape(-1) + 1, torch.full((a * b,), 2)], 1)
            tbl = ops.rulebook_subm(idx.int().to(d), [a + 2, b + 2, 4], 1, 3)
            tb, n = ops.tilebook_build(tbl), tbl.shape[1]
            n_in = n
        else:
            n, n_in, tb = rows, n_in or rows, None
            tbl = torch.randint(-1, n_in, (K, n), generator=g, dtype=torch.int32).to(d)
        x = torch.randn(n_in, kc, generator=g).to(d).to(torch.float32 if esz == 4 else torch.bfloat16)
        w = (torch.randn(K, kc, nc, generator=g) * 0.1).bfloat16().float().to(d)     # bf16-representable: products exact
        xd, wd, t = x.double().cpu(), w.double().cpu(), tbl.cpu().long()
        ref = torch.zeros(n, nc, dtype=torch.float64)
        for o in range(K):
            sel = t[o] >= 0
            ref[sel] += xd[t[o][sel]] @ wd[o]
        for out32 in ((False,) if esz == 4 else (False, True)):
            y = ops.spconv_gather(x, w, tbl, n, 0, nc, out_f32=out32, tilebook=tb).double().cpu()
            print(json.dumps({"family": family, "rows": n, "fp32_out": bool(out32 or esz == 4),
                              "err": float((y - ref).abs().max() / ref.abs().max())}), flush=True)


def instantiations(objs, stem="conv_"):
    """The kernel symbols of compiled objects whose name starts with `stem` (a string or a tuple of them), normalised and sorted:
    conv_* of doda_amd/csrc/_obj/spconv_{gather,tile,wlds}.o is the content of tests/data/gather_instantiations.json,
    wgrad_multi_kernel of spconv_wgrad.o that of tests/data/wgrad_instantiations.json, bn_* and lay_* of bn.o and layers.o that of
    tests/data/bn_instantiations.json."""
    import glob
    import subprocess
    import tempfile
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    names = set()
    for obj in objs:
        with tempfile.TemporaryDirectory() as tmp:
            local = os.path.join(tmp, "in.o")
            with open(obj, "rb") as f, open(local, "wb") as g:
                g.write(f.read())
            subprocess.run([objdump, "--offloading", local], cwd=tmp, capture_output=True)
            for dev in glob.glob(os.path.join(tmp, "*gfx950*")):
                out = subprocess.run([objdump, "-t", "-C", dev], capture_output=True, text=True, check=True).stdout
                for l in out.splitlines():
                    m = re.search(r"\sF \.text\s+\S+\s+(?:\.\w+ )?(.*)$", l)
                    if m and normalise(m.group(1).strip()).startswith(stem):
                        names.add(normalise(m.group(1).strip()))
    return sorted(names)


def normalise(name):
    """A kernel name of the trace without namespaces, argument list and return type."""
    name = name.replace("(anonymous namespace)::", "")
    name = re.sub(r"^void ", "", name)
    m = re.match(r"^([A-Za-z_0-9]+(<.*>)?)\(", name)
    return m.group(1) if m else re.sub(r"\(.*$", "", name)


def fold(trace_csv, results):
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    ev = []
    for r in rows:
        n = normalise(r["Kernel_Name"])
        if re.match(r"^(pack_weights|conv_(fast|gather|tile|tile16|up32|wlds48)\b)", n):
            wg = int(r["Workgroup_Size_X"])
            ev.append((n, int(r["Grid_Size_X"]) // wg, wg))
    res = [json.loads(l) for l in open(results) if l.startswith("{")]
    out, k = [], 0
    for r in res:
        rec = {"name": r["name"], "status": r["status"], "parts": r["rows"], "kernel": None, "grid": 0, "block": 0, "pack": None}
        if r["status"] == 0:
            if ev[k][0].startswith("pack_weights"):
                rec["pack"] = [ev[k][0], ev[k][1], ev[k][2]]
                k += 1
            assert ev[k][0].startswith("conv_"), (r["name"], ev[k])
            rec["kernel"], rec["grid"], rec["block"] = ev[k]
            k += 1
        out.append(rec)
    return out


if __name__ == "__main__":
    if sys.argv[1] == "--run":
        run(sys.argv[2], int(sys.argv[sys.argv.index("--max-rows") + 1]) if "--max-rows" in sys.argv else 1 << 30)
    elif sys.argv[1] == "--numerics":
        os.environ["DODA_TRACE_GATHER"] = "1"       # (read by the library at its first gather call)
        os.environ.pop("DODA_F32_SPLIT_ROWS", None)
        if sys.argv[2] == "f32split":
            os.environ["DODA_F32_SPLIT_ROWS"] = "0"
        import gathernumerics
        gathernumerics.run_group(sys.argv[2])
    elif sys.argv[1] == "--families":
        families()
    elif sys.argv[1] == "--instantiations":
        stem, objs = (tuple(sys.argv[3].split(",")), sys.argv[4:]) if sys.argv[2] == "--stem" else ("conv_", sys.argv[2:])
        print(json.dumps(instantiations(objs, stem), indent=0))
    elif sys.argv[1] == "--fold":
        print(json.dumps(fold(sys.argv[2], sys.argv[3]), indent=0))
