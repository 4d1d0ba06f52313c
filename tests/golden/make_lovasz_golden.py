"""Generates tests/golden/lovasz_golden.npz in the BUILD container (needs /root/reference).

    python tests/golden/make_lovasz_golden.py

The reference's own util/lovasz_loss.py is loaded from where it lies, by file path, and run on the CPU in fp32 (fed fp64 it raises a
dtype error in torch.dot) through autograd: loss = lovasz_softmax(softmax(z[p2v], 1), labels, ignore=255) with the gradient taken
to the VOXEL logits z.  Nothing of its text is copied — the file holds numbers only, per case of tests/lovasz_cases.py (inputs are
regenerated from the seeds, not stored):

    loss_<i>       the reference's loss (fp32)
    dz_<i>         its gradient with respect to z, fp32 [m, n_cls]
    dist_loss_<i>  |reference loss - doda_amd.lovasz.lovasz_softmax in fp64 on the same logits|
    dist_dz_<i>    ||reference dz - fp64 dz|| / ||fp64 dz||   (the reference's own fp32 rounding)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = "/root/reference/util/lovasz_loss.py"

import lovasz_cases as lc   # noqa: E402


def main():
    spec = importlib.util.spec_from_file_location("ref_lovasz_loss", REF)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    from doda_amd.lovasz import lovasz_softmax
    out = {}
    for i in range(lc.N_CASES):
        c = lc.make_case(i)
        p2v, labels = torch.from_numpy(c["p2v"]), torch.from_numpy(c["labels"])
        z32 = torch.from_numpy(c["z"]).float().requires_grad_(True)
        loss = ref.lovasz_softmax(torch.softmax(z32[p2v], 1), labels, ignore=lc.IGNORE)
        loss.backward()
        z64 = torch.from_numpy(c["z"]).requires_grad_(True)
        l64 = lovasz_softmax(z64[p2v], labels, lc.IGNORE)
        l64.backward()
        out["loss_%d" % i] = np.float32(loss.item())
        out["dz_%d" % i] = z32.grad.numpy().astype(np.float32)
        out["dist_loss_%d" % i] = np.float64(abs(float(loss.detach()) - float(l64.detach())))
        out["dist_dz_%d" % i] = np.float64(float((z32.grad.double() - z64.grad).norm() / z64.grad.norm()))
        print("case %d: m %5d classes %2d valid %6d  loss %.7f  fp64 %.9f  dist loss %.2e  dz %.2e" % (
            i + 1, c["m"], c["n_cls"], c["n_valid"], float(loss), float(l64), out["dist_loss_%d" % i], out["dist_dz_%d" % i]))
    path = os.path.join(HERE, "lovasz_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
