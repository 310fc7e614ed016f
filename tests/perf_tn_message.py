"""Microbench (not a test): within-process A/B of the fused TensorNet
message-pass kernels against the torch composition, at the li100k scale.
Run on a GPU box:
    python tests/perf_tn_message.py [--out profiles/tn_message_ab.json]

One GPU graph build of the li100k workload at cutoff 5 gives the true N and
E; the kernel A/B then runs on a Poisson-degree graph of that size with
random senders (no locality to flatter the gathers) and on the built graph
itself, C = 64.  HIP-event medians; bytes/s from the algorithmic traffic
  forward / reverse-node: E*(3C + 9C)*4 + N*9C*4
  reverse-edge:           E*(9C + 3C)*4 + N*9C*4
set against the 6.29 TB/s measured float4-copy ceiling of the MI355X.  One
full engine step at that size with each formulation closes the report.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_CEILING = 6.29e12
C = 64


class _PD:
    pass


def _poisson_graph(N, E, dev, seed=0):
    rng = np.random.default_rng(seed)
    deg = np.maximum(rng.poisson(E / N, N), 1)
    dst = np.repeat(np.arange(N), deg)
    src = rng.integers(0, N, len(dst))
    perm = np.argsort(src, kind="stable")
    pd = _PD()
    i32 = lambda a: torch.as_tensor(a).to(torch.int32).to(dev)  # noqa: E731
    pd.src, pd.dst = i32(src), i32(dst)
    pd.row_ptr = i32(np.concatenate(([0], np.cumsum(deg))))
    pd.src_perm = i32(perm)
    pd.src_row_ptr = i32(np.concatenate(
        ([0], np.cumsum(np.bincount(src, minlength=N)))))
    pd.n_atoms = N
    return pd


def _median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = []
    for _ in range(reps):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        evs.append((s, e))
    torch.cuda.synchronize()
    ts = sorted(s.elapsed_time(e) for s, e in evs)
    return ts[len(ts) // 2]


def _kernel_ab(pd, dev, reps):
    from distmlip_amd.ops import HipOps, _fp, _ip, _stream, hip_lib
    from distmlip_amd.tensornet_ops import tn_message, tn_message_hip
    lib, ops = hip_lib(), HipOps()
    N, E = pd.n_atoms, pd.src.shape[0]
    g = torch.Generator(device=dev).manual_seed(0)
    Y = torch.randn(N, 9, C, device=dev, generator=g)
    f = torch.randn(E, 3, C, device=dev, generator=g)
    G = torch.randn(N, 9, C, device=dev, generator=g)
    M, df, dY = torch.empty_like(Y), torch.empty_like(f), torch.empty_like(Y)

    def fwd():
        assert lib.dm_tn_msg_fwd_f32(_fp(Y), _fp(f), _ip(pd.src),
                                     _ip(pd.row_ptr), _fp(M), N, C,
                                     _stream()) == 0

    def bwd_edge():
        assert lib.dm_tn_msg_bwd_edge_f32(_fp(G), _fp(Y), _ip(pd.src),
                                          _ip(pd.row_ptr), _fp(df), N, C,
                                          _stream()) == 0

    def bwd_node():
        assert lib.dm_tn_msg_bwd_node_f32(_fp(G), _fp(f), _ip(pd.dst),
                                          _ip(pd.src_perm),
                                          _ip(pd.src_row_ptr), _fp(dY), N, C,
                                          _stream()) == 0

    b_node = E * 12 * C * 4 + N * 9 * C * 4
    b_edge = E * 12 * C * 4 + N * 9 * C * 4
    out = {"N": N, "E": E, "C": C, "fused": {}, "torch": {}}
    for name, fn, nbytes in (("fwd", fwd, b_node), ("bwd_edge", bwd_edge,
                                                    b_edge),
                             ("bwd_node", bwd_node, b_node)):
        ms = _median_ms(fn, reps)
        out["fused"][name] = {
            "ms": ms, "bytes": nbytes, "TB_per_s": nbytes / ms * 1e-9,
            "share_of_copy_ceiling": nbytes / (ms * 1e-3) / COPY_CEILING}
    out["fused"]["total_ms"] = sum(out["fused"][k]["ms"]
                                   for k in ("fwd", "bwd_edge", "bwd_node"))

    Yr, fr = Y.clone().requires_grad_(True), f.clone().requires_grad_(True)

    def both(fn):
        Mx = fn()
        torch.autograd.grad(Mx, [Yr, fr], G)

    t_f = _median_ms(lambda: tn_message(Yr, fr, pd, ops), reps)
    t_fb = _median_ms(lambda: both(lambda: tn_message(Yr, fr, pd, ops)),
                      reps)
    h_fb = _median_ms(lambda: both(lambda: tn_message_hip(Yr, fr, pd)), reps)
    out["torch"] = {"fwd_ms": t_f, "fwd_bwd_ms": t_fb}
    out["fused"]["fwd_bwd_autograd_ms"] = h_fb
    out["speedup_fwd_bwd"] = t_fb / h_fb
    return out


def _full_step(structure, mode, steps):
    from distmlip_amd.tensornet_model import TensorNetConfig, TensorNetCore
    from distmlip_amd.tensornet_runtime import TensorNetSpmdEngine
    os.environ["DM_TN_MSG"] = mode
    cfg = TensorNetConfig(n_elements=int(structure.species.max()) + 1,
                          units=C)
    eng = TensorNetSpmdEngine(TensorNetCore.seeded(cfg, seed=0), world=1)
    ts, out = [], None
    for i in range(steps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = eng.step(structure)
        torch.cuda.synchronize()
        if i >= 2:
            ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"ms_per_step": ts[len(ts) // 2],
            "peak_mem_GB": torch.cuda.max_memory_allocated() / 1e9,
            "energy": out["energy"].item(),
            "max_abs_force": out["forces_owned"].abs().max().item()}, \
        out["forces_owned"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/tn_message_ab.json")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP GPU"
    dev = torch.device("cuda:0")
    from distmlip_amd import gpu_graph
    from distmlip_amd.structures import workload

    s = workload("li100k")
    built = gpu_graph.build(s, 5.0, 0.0, 1e-8, False, dev)
    N, E = built.n_atoms, int(built.src.shape[0])
    res = {"workload": "li100k", "cutoff": 5.0, "N": N, "E_true": E,
           "edges_per_atom": E / N, "copy_ceiling_TB_per_s": 6.29,
           "timer": "HIP events, median of %d" % a.reps}
    res["poisson_graph"] = _kernel_ab(_poisson_graph(N, E, dev), dev, a.reps)
    res["built_graph"] = _kernel_ab(built, dev, a.reps)
    del built
    torch.cuda.empty_cache()
    res["full_step"] = {}
    forces = {}
    for mode in ("hip", "torch"):
        torch.cuda.reset_peak_memory_stats()
        res["full_step"][mode], forces[mode] = _full_step(s, mode, a.steps)
        torch.cuda.empty_cache()
    res["full_step"]["max_abs_force_diff"] = \
        (forces["hip"] - forces["torch"]).abs().max().item()
    res["fused_is_faster"] = bool(
        res["poisson_graph"]["speedup_fwd_bwd"] > 1.0
        and res["full_step"]["hip"]["ms_per_step"]
        < res["full_step"]["torch"]["ms_per_step"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
