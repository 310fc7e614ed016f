"""Microbench (not a test): the whole gated MLP in one kernel
(dm_gated_mlp3/4_f32) against the pair it replaces (dm_edge_mlp3/4_f32 +
dm_gated_mlp_tail_fwd_f32), form by form, on random inputs at the si1m row
counts.  Node tables of 1M rows; dst is sorted with degree 46, src and the
third index fall within +-4096 rows of dst (the slab-spatial locality of a
built graph).  Median and spread of 5 launches after one warm-up, outputs
preallocated.  Run on a GPU:
    python tests/perf_gated_mlp_fused.py [out.json]
"""
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D = 64
N_TABLE = 1_000_000
HBM = 6.29e12          # achievable bytes/s, the figure of the kernel headers
MFMA = 157e12          # fp32 MFMA peak, flop/s


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


def fp(t, off=0):
    if t is None:
        return None
    return ctypes.cast(t.data_ptr() + 4 * off, ctypes.POINTER(ctypes.c_float))


def ip(t):
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_int32))


def main():
    from distmlip_amd.ops import _stream, hip_lib
    lib = hip_lib()
    dev = torch.device("cuda:0")
    res = {}
    for name, E in (("46M", 46_000_000), ("12M", 12_000_000)):
        r = {"rows": E,
             "floor_ms_mfma": round(2 * 2 * E * D * 2 * D / MFMA * 1e3, 2)}
        row = torch.randn(E, D, device=dev)
        wt = torch.randn(D, 2 * D, device=dev) / 8
        bias = torch.randn(2 * D, device=dev)
        tabs = [torch.randn(N_TABLE, 2 * D, device=dev) for _ in range(3)]
        dst = (torch.arange(E, device=dev) // 46).clamp_(max=N_TABLE - 1)
        near = [(dst + torch.randint(-4096, 4097, (E,), device=dev)).clamp_(
            0, N_TABLE - 1).to(torch.int32) for _ in range(2)]
        idx = [near[0], dst.to(torch.int32), near[1]]
        del dst
        w2 = torch.randn(2, D, D, device=dev) / 8
        b2 = torch.randn(2, 1, D, device=dev)
        w = torch.randn(E, D, device=dev)
        base = torch.randn(E, D, device=dev)
        z = torch.empty(E, 2 * D, device=dev)
        h = torch.empty(E, 2 * D, device=dev)
        cg = torch.empty(2, E, D, device=dev)
        out = torch.empty(E, D, device=dev)
        second = (fp(w2), fp(w2, D * D), fp(b2), fp(b2, D))

        def first(ng, keep):
            if ng == 2:
                return lib.dm_edge_mlp3_f32(
                    fp(row), fp(wt), fp(bias), fp(tabs[0]), fp(tabs[1]),
                    ip(idx[0]), ip(idx[1]), fp(z) if keep else None, fp(h), E,
                    D, 2 * D, _stream())
            return lib.dm_edge_mlp4_f32(
                fp(row), fp(wt), fp(bias), fp(tabs[0]), fp(tabs[1]),
                fp(tabs[2]), ip(idx[0]), ip(idx[1]), ip(idx[2]),
                fp(z) if keep else None, fp(h), E, D, 2 * D, _stream())

        def tail(keep, w_, base_):
            return lib.dm_gated_mlp_tail_fwd_f32(
                fp(h), *second, fp(w_), fp(base_),
                fp(cg) if keep else None, fp(cg, E * D) if keep else None,
                fp(out), E, D, _stream())

        def fused(ng, keep, want_out, w_, base_):
            outs = (fp(z) if keep else None, fp(cg) if keep else None,
                    fp(cg, E * D) if keep else None,
                    fp(out) if want_out else None, E, D, D, _stream())
            if ng == 2:
                return lib.dm_gated_mlp3_f32(
                    fp(row), fp(wt), fp(bias), fp(tabs[0]), fp(tabs[1]),
                    ip(idx[0]), ip(idx[1]), *second, fp(w_), fp(base_), *outs)
            return lib.dm_gated_mlp4_f32(
                fp(row), fp(wt), fp(bias), fp(tabs[0]), fp(tabs[1]),
                fp(tabs[2]), ip(idx[0]), ip(idx[1]), ip(idx[2]), *second,
                fp(w_), fp(base_), *outs)

        def must(rc):
            assert rc == 0, lib.dm_hip_last_error()

        for ng in (2, 3):
            rows = E * D * 4
            # (form, keep, want_out, w, base, [E,64] arrays the result needs)
            forms = (("nokeep_w_base", False, True, w, base, 4),
                     ("nokeep_w", False, True, w, None, 3),
                     ("keep_w_base", True, True, w, base, 8),
                     ("keep_w", True, True, w, None, 7),
                     # the pair has no out-less form: it computes out from w
                     ("keep_noout", True, False, w, None, 5))
            for form, keep, want_out, w_, base_, arrays in forms:
                def pair():
                    must(first(ng, keep))
                    must(tail(keep, w_, base_))
                one = timed(lambda: must(fused(
                    ng, keep, want_out, w_ if want_out else None,
                    base_ if want_out else None)))
                two = timed(pair)
                spread = max(one["max_ms"] - one["min_ms"],
                             two["max_ms"] - two["min_ms"])
                r[f"ng{ng}_{form}"] = {
                    "fused": one, "pair": two,
                    "gain_ms": round(two["median_ms"] - one["median_ms"], 3),
                    "wins": bool(two["min_ms"] - one["max_ms"] > 0
                                 and two["median_ms"] - one["median_ms"]
                                 > spread),
                    "floor_ms_bytes": round(arrays * rows / HBM * 1e3, 2)}
            r[f"ng{ng}_first_noz"] = timed(lambda: must(first(ng, False)))
            r[f"ng{ng}_first_z"] = timed(lambda: must(first(ng, True)))
        res[name] = r
        print(name, json.dumps(r), flush=True)
        del row, tabs, idx, near, w, base, z, h, cg, out
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
