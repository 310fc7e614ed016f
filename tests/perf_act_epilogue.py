"""Microbench (not a test): what the exact sigmoid / SiLU costs in the fp32-MFMA
gated-MLP kernels, and the ceiling of what trimming it can buy.  Three scratch
copies of the kernel library are timed on the same inputs:
  ref    -DDM_ACT_REF         1/(1+expf(-x)), x/(1+expf(-x)) as the compiler
                              emits them (25 VALU instructions each)
  new    (no define)          the short sequences of csrc/kernels.hip
  free   -DDM_ACT_PROBE_FREE  both functions return x: WRONG results, timed
                              only; what is left is the kernel without any
                              activation arithmetic
The copies are built into build/act_epilogue/ (hipcc, the Makefile's flags) if
they are not there yet.  Forms: the launches of one si1m step that evaluate the
functions, plus k_edge_mlp_bwd, which evaluates none and must not move.  Random
inputs at the si1m row counts, node tables of 1M rows, dst sorted with degree
46, the other index within +-4096 rows of it.  Median, min and max of 5
launches after one warm-up per build, builds alternating form by form.
Run on a GPU:
    python tests/perf_act_epilogue.py [out.json]
"""
import ctypes
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distmlip_amd", "csrc")
OUT = os.path.join(ROOT, "build", "act_epilogue")
BUILDS = (("ref", ["-DDM_ACT_REF"]), ("new", []),
          ("free", ["-DDM_ACT_PROBE_FREE"]))
SRCS = ("kernels.hip", "tensornet.hip", "md.hip", "rows.hip")

D = 64
N_RBF = 9
N_TABLE = 1_000_000
HBM = 6.29e12          # achievable bytes/s, the figure of the kernel headers
MFMA = 157e12          # fp32 MFMA peak, flop/s

i64 = ctypes.c_int64


def build_libs():
    os.makedirs(OUT, exist_ok=True)
    libs = {}
    for name, defs in BUILDS:
        path = os.path.join(OUT, f"libdistmlip_hip_{name}.so")
        if not os.path.exists(path):
            subprocess.run(
                ["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                 "-fPIC", "-shared", *defs,
                 *(os.path.join(CSRC, s) for s in SRCS), "-o", path],
                check=True)
        lib = ctypes.CDLL(path)
        lib.dm_hip_last_error.restype = ctypes.c_char_p
        libs[name] = lib
    return libs


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
    libs = build_libs()
    dev = torch.device("cuda:0")

    def stream():
        return ctypes.c_uint64(torch.cuda.current_stream().cuda_stream)

    res = {}
    for name, E in (("46M", 46_000_000), ("12M", 12_000_000)):
        rows = E * D * 4               # bytes of one [E,64] array
        tile_mfma = 2 * E * D * 2 * D / MFMA * 1e3     # one [E,64]x[64,128]
        bexp = torch.randn(E, N_RBF, device=dev)
        W = torch.randn(D, N_RBF, device=dev) / 3
        dbexp = torch.zeros(E, N_RBF, device=dev)
        h = torch.randn(E, 2 * D, device=dev)       # also z of the reverse
        zbuf = torch.empty(E, 2 * D, device=dev)    # z_out / dz / h out
        cg = torch.randn(2, E, D, device=dev)
        cg_out = torch.empty(2, E, D, device=dev)
        base = torch.randn(E, D, device=dev)        # also erow, go and gbase
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
        gathers = (fp(base), fp(wt), fp(bias), fp(tabs[0]), fp(tabs[1]),
                   ip(src), ip(dst))
        keeps = (fp(zbuf), fp(cg_out), fp(cg_out, E * D))
        dims = (i64(E), i64(D), i64(D))

        def mlp_fw(lib, base_):
            return lib.dm_gated_mlp3_fw_f32(
                *gathers, *second, fp(bexp), fp(W), None, fp(base_), *keeps,
                fp(out), *dims, i64(N_RBF), stream())

        def mlp_noout(lib):
            return lib.dm_gated_mlp3_f32(
                *gathers, *second, None, None, *keeps, None, *dims, stream())

        def bwd_fw(lib, indexed):
            return lib.dm_gated_mlp_tail_bwd_fw_f32(
                fp(go_tab) if indexed else fp(base),
                ip(dst) if indexed else None, fp(cg), fp(cg, E * D), fp(bexp),
                fp(W), None, fp(h), fp(w2), fp(w2, D * D), fp(zbuf),
                None if indexed else fp(dbexp), fp(dbexp), i64(E), i64(D),
                i64(N_RBF), stream())

        def first_noz(lib):
            return lib.dm_edge_mlp3_f32(
                *gathers, None, fp(zbuf), i64(E), i64(D), i64(2 * D),
                stream())

        def tail_fw(lib, base_):
            return lib.dm_gated_mlp_tail_fwd_fw_f32(
                fp(h), *second, fp(bexp), fp(W), None, fp(base_), None, None,
                fp(out), i64(E), i64(D), i64(N_RBF), stream())

        def first_bwd(lib):
            return lib.dm_edge_mlp_bwd_f32(
                fp(h), fp(wt), fp(base), fp(out), i64(E), i64(2 * D), i64(D),
                stream())

        # (form, launch, [E,64] arrays moved, [E,64]x[64,128] products,
        #  activations per row)
        forms = (
            ("mlp3_keep_fw_base", lambda l: mlp_fw(l, base), 7.14, 2, 256),
            ("mlp3_keep_fw", lambda l: mlp_fw(l, None), 6.14, 2, 256),
            ("mlp3_keep_noout", mlp_noout, 5, 2, 128),
            ("tail_bwd_fw", lambda l: bwd_fw(l, False), 7.42, 1, 256),
            ("tail_bwd_fw_idx", lambda l: bwd_fw(l, True), 6.28, 1, 256),
            ("edge_mlp3_noz", first_noz, 3, 1, 128),
            ("tail_fwd_fw_base", lambda l: tail_fw(l, base), 4.14, 1, 128),
            ("tail_fwd_fw", lambda l: tail_fw(l, None), 3.14, 1, 128),
            ("edge_mlp_bwd_control", first_bwd, 4, 1, 0),
        )
        r = {"rows": E}
        for form, launch, arrays, products, acts in forms:
            entry = {"floor_ms_bytes": round(arrays * rows / HBM * 1e3, 2),
                     "floor_ms_mfma": round(products * tile_mfma, 2),
                     "activations_per_row": acts}
            for build, lib in libs.items():
                def run():
                    rc = launch(lib)
                    assert rc == 0, lib.dm_hip_last_error()
                entry[build] = timed(run)
            entry["new_minus_ref_ms"] = round(
                entry["new"]["median_ms"] - entry["ref"]["median_ms"], 3)
            entry["free_minus_ref_ms"] = round(
                entry["free"]["median_ms"] - entry["ref"]["median_ms"], 3)
            r[form] = entry
            print(name, form, json.dumps(entry), flush=True)
        res[name] = r
        del bexp, dbexp, h, zbuf, cg, cg_out, base, out, tabs, go_tab, dst, src
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
