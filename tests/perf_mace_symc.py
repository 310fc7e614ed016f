"""Microbench (not a test): the tree-factored MACE symmetric contraction
(csrc/mace_symc.hip) against what served the same inputs before it, on 64 000
nodes, both product shapes, forward and forward + reverse through autograd.
At C = 128 the other side is the flat kernel (dm_mace_symc_*), at C = 192 and
256 the fp32 torch composition.  Run on a GPU box:
    python tests/perf_mace_symc.py [--out profiles/mace_symc_tree_standalone.json]

HIP-event medians.  The kernels are bound by LDS and VALU issue, not by
memory: the compulsory traffic (N*(16 + S_out)*C*4 bytes per pass, twice that
in the reverse) is listed with its share of the 6.29 TB/s copy ceiling only to
show how far from it they run.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.perf_tn_message import COPY_CEILING, _median_ms  # noqa: E402

N = 64000


def _shape_ab(prod, corr, C, other, dev, reps):
    from distmlip_amd import mace_ops
    g = torch.Generator(device=dev).manual_seed(C)
    x = {l: torch.randn(N, C, 2 * l + 1, device=dev, generator=g)
         .requires_grad_(True) for l in range(4)}
    species = torch.randint(0, prod.weights["0_1"].shape[0], (N,),
                            device=dev, generator=g)
    S_out = sum(2 * lo + 1 for lo in prod.out_ls)
    cot = [torch.randn(N, C, 2 * lo + 1, device=dev, generator=g)
           for lo in prod.out_ls]
    fns = {"tree": mace_ops.symmetric_contract_tree,
           "flat": mace_ops.symmetric_contract_hip,
           "torch": mace_ops.symmetric_contract}
    sizes = mace_ops._symc_tree_tables(tuple(prod.out_ls), corr, str(dev))[3]
    out = {"out_ls": list(prod.out_ls), "table": sizes,
           "bytes_fwd": N * (16 + S_out) * C * 4}
    for name in (other, "tree"):
        if name == "torch":
            os.environ["DM_MACE_SYMC"] = "torch"

        def fwd():
            y = fns[name](prod, x, species, corr)
            return [y[lo] for lo in prod.out_ls]

        def both():
            torch.autograd.grad(fwd(), list(x.values()), cot)

        with torch.no_grad():
            f_ms = _median_ms(fwd, reps)
        out[name] = {"fwd_ms": f_ms}
        try:
            out[name]["fwd_bwd_ms"] = _median_ms(both, reps)
        except torch.OutOfMemoryError:      # the composition's saved arrays
            out[name]["fwd_bwd_ms"] = None
        os.environ.pop("DM_MACE_SYMC", None)
        torch.cuda.empty_cache()
    out["tree"]["fwd_share_of_copy_ceiling"] = (
        out["bytes_fwd"] / (out["tree"]["fwd_ms"] * 1e-3) / COPY_CEILING)
    out["speedup_fwd"] = out[other]["fwd_ms"] / out["tree"]["fwd_ms"]
    if out[other]["fwd_bwd_ms"] is not None:
        out["speedup_fwd_bwd"] = (out[other]["fwd_bwd_ms"]
                                  / out["tree"]["fwd_bwd_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/mace_symc_tree_standalone.json")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP GPU"
    dev = torch.device("cuda:0")
    from distmlip_amd.mace_model import MACEConfig, MACECore

    res = {"nodes": N, "copy_ceiling_TB_per_s": 6.29,
           "timer": "HIP events, median of %d" % a.reps}
    for C, other in ((128, "flat"), (192, "torch"), (256, "torch")):
        core = MACECore.seeded(MACEConfig(n_elements=3, channels=C),
                               seed=0).float().to(dev)
        core.requires_grad_(False)
        for layer, prod in enumerate(core.products):
            res["C%d_layer%d" % (C, layer)] = dict(
                _shape_ab(prod, core.config.correlation, C, other, dev,
                          a.reps), C=C, other=other)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
