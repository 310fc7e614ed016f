"""Microbench (not a test): the first layer's reverse kernel and the indexed
reverse tail against what each replaces, on random inputs at the si1m row
counts.  Median and spread of 5 launches after one warm-up.  Run on a GPU:
    python tests/perf_edge_mlp_bwd.py [out.json]
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D = 64
HBM = 6.29e12          # achievable bytes/s, the figure of the kernel headers


def timed(fn, n=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    ts.sort()
    return {"median_ms": round(ts[n // 2], 3), "min_ms": round(ts[0], 3),
            "max_ms": round(ts[-1], 3)}


def main():
    from distmlip_amd.ops import (raw_edge_mlp_bwd, raw_gather,
                                  raw_mlp_tail_bwd)
    dev = torch.device("cuda:0")
    res = {}
    for name, E in (("46M", 46_000_000), ("12M", 12_000_000)):
        r = {"rows": E}
        dz = torch.randn(E, 2 * D, device=dev)
        wt = torch.randn(D, 2 * D, device=dev) / 8
        gbase = torch.randn(E, D, device=dev)
        out = torch.empty(E, D, device=dev)
        wtt = wt.t()
        r["edge_mlp_bwd_gbase"] = timed(
            lambda: raw_edge_mlp_bwd(dz, wt, gbase, out))
        r["edge_mlp_bwd_gbase_inplace"] = timed(
            lambda: raw_edge_mlp_bwd(dz, wt, out, out))
        r["edge_mlp_bwd"] = timed(lambda: raw_edge_mlp_bwd(dz, wt, None, out))
        r["addmm"] = timed(lambda: torch.addmm(gbase, dz, wtt, out=out))
        r["mm"] = timed(lambda: torch.mm(dz, wtt, out=out))
        r["mm_plus_add"] = timed(
            lambda: torch.add(torch.mm(dz, wtt, out=out), gbase))
        r["floor_ms_gbase"] = round(E * 4 * D * 4 / HBM * 1e3, 2)
        r["floor_ms"] = round(E * 3 * D * 4 / HBM * 1e3, 2)
        del gbase, out

        # indexed tail: dst-sorted index of degree 46 over E/46 table rows
        n = E // 46
        idx = (torch.arange(E, device=dev) // 46).clamp_(max=n - 1).to(
            torch.int32)
        table = torch.randn(n, D, device=dev)
        cg = torch.randn(2, E, D, device=dev)
        w = torch.randn(E, D, device=dev)
        w2 = torch.randn(2, D, D, device=dev) / 8
        z = dz
        r["tail_idx"] = timed(
            lambda: raw_mlp_tail_bwd(table, cg, w, z, w2, idx))
        r["gather_plus_tail"] = timed(
            lambda: raw_mlp_tail_bwd(raw_gather(table, idx), cg, w, z, w2))
        r["gather"] = timed(lambda: raw_gather(table, idx))
        res[name] = r
        print(name, json.dumps(r), flush=True)
        del dz, cg, w, z, idx, table
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
