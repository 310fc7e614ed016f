"""Microbench (not a test): the indexed row moves against the torch ops they
replace, at the si1m shapes: M = 4M rows moved between a table of R = 46M
rows and one of M rows, D = 64, int64 indices (a random subset of the 46M
rows on the edge side, arange on the bond side, as both builders emit).
Median and spread of 5 launches after one warm-up.  Run on a GPU:
    python tests/perf_row_exchange.py [out.json]
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
    from distmlip_amd.ops import raw_move_rows, raw_zero_rows
    dev = torch.device("cuda:0")
    M, R = 4_000_000, 46_000_000
    gen = torch.Generator(device="cpu").manual_seed(1)
    # sorted, as g2l_edge[bde_e] is for a dst-sorted edge list
    map_de = torch.sort(torch.randperm(R, generator=gen)[:M]).values.to(dev)
    map_ude = torch.arange(M, device=dev)
    e = torch.randn(R, D, device=dev)
    n = torch.randn(M, D, device=dev)
    r = {"M": M, "R": R, "D": D,
         "floor_ms_move": round(2 * M * D * 4 / HBM * 1e3, 3),
         "floor_ms_add": round(3 * M * D * 4 / HBM * 1e3, 3),
         "floor_ms_zero": round(M * D * 4 / HBM * 1e3, 3),
         "floor_ms_dense_copy": round(2 * R * D * 4 / HBM * 1e3, 3)}

    # gather e -> n (edge_to_bond forward; bond_to_edge reverse)
    r["move_gather"] = timed(
        lambda: raw_move_rows(e, map_de, n, map_ude))
    r["move_gather_null_di"] = timed(
        lambda: raw_move_rows(e, map_de, n, None))
    r["torch_index"] = timed(lambda: e[map_de])
    r["torch_index_then_index_copy_"] = timed(
        lambda: n.index_copy_(0, map_ude, e[map_de]))
    # scatter n -> e (bond_to_edge forward)
    r["move_scatter"] = timed(
        lambda: raw_move_rows(n, map_ude, e, map_de))
    r["torch_index_copy_"] = timed(
        lambda: e.index_copy_(0, map_de, n[map_ude]))
    r["torch_index_copy_out_of_place"] = timed(
        lambda: e.index_copy(0, map_de, n[map_ude]))
    # add n -> e rows (edge_to_bond reverse)
    r["move_scatter_add"] = timed(
        lambda: raw_move_rows(n, map_ude, e, map_de, add=True))
    r["torch_index_put_accumulate"] = timed(
        lambda: e.index_put_((map_de,), n[map_ude], accumulate=True))
    # zero rows (both reverses)
    r["zero_rows"] = timed(lambda: raw_zero_rows(e, map_de))
    r["torch_index_fill_"] = timed(lambda: e.index_fill_(0, map_de, 0))
    r["zero_rows_bond_side"] = timed(lambda: raw_zero_rows(n, map_ude))
    # the dense copy that stays in each reverse
    r["torch_clone_dense"] = timed(lambda: e.clone())
    print(json.dumps(r), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
