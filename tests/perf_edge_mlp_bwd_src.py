"""Microbench (not a test): the first layer's reverse kernel in src order with
the src segment sums (raw_edge_mlp_bwd_src) against the pair it replaces,
raw_edge_mlp_bwd + raw_seg_sum_gather, on random inputs at the si1m row counts
over a 1M-node table.  The permutation is a real one: a dst-sorted symmetric
index (node i is joined to i +- o_k for a fixed set of offsets), sorted by
src.  Median and spread of 5 launches after one warm-up.  Run on a GPU:
    python tests/perf_edge_mlp_bwd_src.py [out.json] [46M|12M ...]
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from perf_edge_mlp_bwd import D, HBM, timed  # noqa: E402

N_NODES = 1_000_000
M_PATCH = 200_000           # exchanged rows of the patched form
SIZES = {"46M": 46, "12M": 12}      # name -> degree


def graph(degree, dev):
    """(perm, seg, row_ptr) of the src order of a dst-sorted symmetric index
    of the given (even) degree over N_NODES nodes."""
    gen = torch.Generator(device="cpu").manual_seed(degree)
    half = torch.randperm(5000, generator=gen)[:degree // 2] + 1
    off = torch.cat([half, -half]).to(dev)
    dst = torch.arange(N_NODES, device=dev).repeat_interleave(degree)
    src = (dst + off.repeat(N_NODES)) % N_NODES
    perm = torch.argsort(src, stable=True)
    seg = src[perm].to(torch.int32)
    rp = torch.zeros(N_NODES + 1, dtype=torch.int32, device=dev)
    rp[1:] = torch.cumsum(torch.bincount(src, minlength=N_NODES), 0)
    return perm.to(torch.int32), seg, rp


def main():
    from distmlip_amd.ops import (raw_edge_mlp_bwd, raw_edge_mlp_bwd_src,
                                  raw_seg_sum_gather)
    dev = torch.device("cuda:0")
    names = sys.argv[2:] or list(SIZES)
    res = {}
    for name in names:
        perm, seg, rp = graph(SIZES[name], dev)
        E = perm.shape[0]
        r = {"rows": E, "nodes": N_NODES}
        dz = torch.randn(E, 2 * D, device=dev)
        wt = torch.randn(D, 2 * D, device=dev) / 8
        gbase = torch.randn(E, D, device=dev)
        out = torch.empty(E, D, device=dev)
        rows = torch.randn(M_PATCH, D, device=dev)
        slot = torch.full((E,), -1, dtype=torch.int32, device=dev)
        slot[torch.randperm(E, device=dev)[:M_PATCH]] = torch.arange(
            M_PATCH, dtype=torch.int32, device=dev)
        order = (perm, seg, rp)
        forms = {"": (None, None), "_gbase": (gbase, None),
                 "_patch": (gbase, (slot, rows))}
        for tag, (gb, patch) in forms.items():
            r["src" + tag] = timed(lambda: raw_edge_mlp_bwd_src(
                dz, wt, *order, gb, out, patch))
            r["pair" + tag] = timed(lambda: (
                raw_edge_mlp_bwd(dz, wt, gb, out, patch),
                raw_seg_sum_gather(dz, perm, rp, N_NODES)))
            r["plain" + tag] = timed(
                lambda: raw_edge_mlp_bwd(dz, wt, gb, out, patch))
        r["src_gbase_inplace"] = timed(lambda: raw_edge_mlp_bwd_src(
            dz, wt, *order, out, out))
        r["gather"] = timed(
            lambda: raw_seg_sum_gather(dz, perm, rp, N_NODES))
        r["floor_ms_gbase"] = round(E * 4 * D * 4 / HBM * 1e3, 2)
        r["floor_ms"] = round(E * 3 * D * 4 / HBM * 1e3, 2)
        res[name] = r
        print(name, json.dumps(r), flush=True)
        del dz, gbase, out, slot, perm, seg
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
