"""Microbench (not a test): the factored-w forms of the gated-MLP kernels
(dm_gated_mlp_tail_fwd_fw_f32, dm_gated_mlp3_fw_f32,
dm_gated_mlp_tail_bwd_fw_f32) against what each replaces in an atom-conv
block, on random inputs at the si1m row counts:
  forward forms   the GEMM that builds w = bexp @ W.t() + the dense kernel
  reverse forms   that GEMM + the dense kernel + the GEMM dbexp (+)= dw @ W
Node table of 1M rows, dst sorted with degree 46 (the indexed reverse form
and the whole-MLP gathers).  Median and spread of 5 launches after one
warm-up, outputs preallocated.  A form wins when it beats what it replaces by
more than both spreads.  Run on a GPU:
    python tests/perf_factored_w.py [out.json [form-prefix]]
"""
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D = 64
N_RBF = 9
N_TABLE = 1_000_000
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


def fp(t, off=0):
    if t is None:
        return None
    return ctypes.cast(t.data_ptr() + 4 * off, ctypes.POINTER(ctypes.c_float))


def ip(t):
    if t is None:
        return None
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_int32))


def main():
    from distmlip_amd.ops import _stream, hip_lib
    lib = hip_lib()
    dev = torch.device("cuda:0")
    only = sys.argv[2] if len(sys.argv) > 2 else ""
    res = {}
    for name, E in (("46M", 46_000_000), ("12M", 12_000_000)):
        rows = E * D * 4               # bytes of one [E,64] array
        r = {"rows": E}
        bexp = torch.randn(E, N_RBF, device=dev)
        W = torch.randn(D, N_RBF, device=dev) / 3
        mask = (torch.rand(E, device=dev) < 0.8).float()
        w = torch.empty(E, D, device=dev)           # the dense weight
        dw = torch.empty(E, D, device=dev)
        dbexp = torch.zeros(E, N_RBF, device=dev)
        h = torch.randn(E, 2 * D, device=dev)       # also z of the reverse
        zbuf = torch.empty(E, 2 * D, device=dev)    # z_out / dz
        cg = torch.randn(2, E, D, device=dev)
        base = torch.randn(E, D, device=dev)        # also erow and go
        out = torch.empty(E, D, device=dev)
        w2 = torch.randn(2, D, D, device=dev) / 8
        b2 = torch.randn(2, 1, D, device=dev)
        wt = torch.randn(D, 2 * D, device=dev) / 8
        bias = torch.randn(2 * D, device=dev)
        tabs = [torch.randn(N_TABLE, 2 * D, device=dev) for _ in range(2)]
        go_tab = torch.randn(N_TABLE, D, device=dev)
        dst = (torch.arange(E, device=dev) // 46).clamp_(max=N_TABLE - 1)
        src = (dst + torch.randint(-4096, 4097, (E,), device=dev)).clamp_(
            0, N_TABLE - 1).to(torch.int32)
        dst = dst.to(torch.int32)
        second = (fp(w2), fp(w2, D * D), fp(b2), fp(b2, D))
        Wt = W.t()

        def must(rc):
            assert rc == 0, lib.dm_hip_last_error()

        def build_w():
            torch.mm(bexp, Wt, out=w)

        def tail_dense(base_):
            build_w()
            must(lib.dm_gated_mlp_tail_fwd_f32(
                fp(h), *second, fp(w), fp(base_), None, None, fp(out), E, D,
                _stream()))

        def tail_fw(base_, mask_):
            must(lib.dm_gated_mlp_tail_fwd_fw_f32(
                fp(h), *second, fp(bexp), fp(W), fp(mask_), fp(base_), None,
                None, fp(out), E, D, N_RBF, _stream()))

        gathers = (fp(base), fp(wt), fp(bias), fp(tabs[0]), fp(tabs[1]),
                   ip(src), ip(dst))
        keeps = (fp(zbuf), fp(cg), fp(cg, E * D), fp(out))

        def mlp_dense():
            build_w()
            must(lib.dm_gated_mlp3_f32(
                *gathers, *second, fp(w), fp(base), *keeps, E, D, D,
                _stream()))

        def mlp_fw(mask_):
            must(lib.dm_gated_mlp3_fw_f32(
                *gathers, *second, fp(bexp), fp(W), fp(mask_), fp(base),
                *keeps, E, D, D, N_RBF, _stream()))

        def bwd_dense(indexed):
            build_w()
            if indexed:
                must(lib.dm_gated_mlp_tail_bwd_idx_f32(
                    fp(go_tab), ip(dst), fp(cg), fp(cg, E * D), fp(w), fp(h),
                    fp(w2), fp(w2, D * D), fp(zbuf), fp(dw), E, D, _stream()))
                torch.mm(dw, W, out=dbexp)
            else:
                must(lib.dm_gated_mlp_tail_bwd_f32(
                    fp(base), fp(cg), fp(cg, E * D), fp(w), fp(h), fp(w2),
                    fp(w2, D * D), fp(zbuf), fp(dw), E, D, _stream()))
                dbexp.addmm_(dw, W)

        def bwd_fw(indexed, mask_):
            # the node MLP's launch (indexed) starts dbexp, the edge MLP's
            # (plain) accumulates onto it in place
            must(lib.dm_gated_mlp_tail_bwd_fw_f32(
                fp(go_tab) if indexed else fp(base),
                ip(dst) if indexed else None, fp(cg), fp(cg, E * D), fp(bexp),
                fp(W), fp(mask_), fp(h), fp(w2), fp(w2, D * D), fp(zbuf),
                None if indexed else fp(dbexp), fp(dbexp), E, D, N_RBF,
                _stream()))

        # (form, dense chain, factored, factored with mask, [E,64]-array
        #  equivalents the factored form moves, dense-only extra arrays)
        forms = (
            ("tail_fwd_nokeep_w_base", lambda: tail_dense(base),
             lambda: tail_fw(base, None), lambda: tail_fw(base, mask), 4),
            ("tail_fwd_nokeep_w", lambda: tail_dense(None),
             lambda: tail_fw(None, None), lambda: tail_fw(None, mask), 3),
            ("mlp3_keep_w_base", mlp_dense, lambda: mlp_fw(None),
             lambda: mlp_fw(mask), 7),
            ("tail_bwd", lambda: bwd_dense(False),
             lambda: bwd_fw(False, None), lambda: bwd_fw(False, mask), 7),
            ("tail_bwd_idx", lambda: bwd_dense(True),
             lambda: bwd_fw(True, None), lambda: bwd_fw(True, mask), 6),
        )
        for form, dense, fw, fw_mask, arrays in forms:
            if not form.startswith(only):
                continue
            one, two = timed(fw), timed(dense)
            spread = max(one["max_ms"] - one["min_ms"],
                         two["max_ms"] - two["min_ms"])
            r[form] = {
                "factored": one, "factored_masked": timed(fw_mask),
                "dense_chain": two,
                "gain_ms": round(two["median_ms"] - one["median_ms"], 3),
                "wins": bool(two["min_ms"] - one["max_ms"] > 0
                             and two["median_ms"] - one["median_ms"] > spread),
                "floor_ms_bytes": round(
                    (arrays * rows + E * N_RBF * 4) / HBM * 1e3, 2)}
        r["gemm_w"] = timed(build_w)
        r["gemm_dbexp"] = timed(lambda: torch.mm(dw, W, out=dbexp))
        res[name] = r
        print(name, json.dumps(r), flush=True)
        del bexp, w, dw, dbexp, h, zbuf, cg, base, out, tabs, go_tab, dst, src
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
