"""Microbench (not a test): the fused MACE convolution kernels against the
ops they replace (gather + dm_mace_tp_* + four segment sums, and their
reverse), on the graph of the mace62k workload, C = 128.  Run on a GPU box:
    python tests/perf_mace_conv.py [--out profiles/mace_conv_standalone.json]

HIP-event medians; bytes/s from the compulsory traffic per pass, with every
node row (xs, M or G, dxs) counted once, since re-reads of sender rows are
served by the caches,
  fwd, bwd_node: E*(P*C + 16)*4 + N*(R + 16)*C*4
  bwd_edge:      E*(2*P*C + 16 + 16*C/64)*4 + N*(R + 16)*C*4
set against the 6.29 TB/s measured float4-copy ceiling of the MI355X.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.perf_tn_message import COPY_CEILING, _median_ms  # noqa: E402

C = 128


def _layer_ab(layer, inter, pd, dev, reps):
    from distmlip_amd import mace_ops
    from distmlip_amd.ops import HipOps, _fp, _ip, _stream, hip_lib
    lib, ops = hip_lib(), HipOps()
    N, E, P, R = pd.n_atoms, pd.src.shape[0], len(inter.paths), (1, 4)[layer]
    g = torch.Generator(device=dev).manual_seed(layer)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    x = {l: rnd(N, C, 2 * l + 1).requires_grad_(True)
         for l in range(layer + 1)}
    Y, w = rnd(E, 16).requires_grad_(True), rnd(E, P, C).requires_grad_(True)
    G = {l3: rnd(N, C, 2 * l3 + 1) for l3 in range(4)}
    leaves = list(x.values()) + [Y, w]

    def split():
        flat = lambda t: t.reshape(t.shape[0], -1).contiguous()  # noqa: E731
        gath = {l: ops.gather(flat(t), pd.src, csr=(pd.src_perm,
                                                    pd.src_row_ptr)
                              ).view(-1, C, 2 * l + 1) for l, t in x.items()}
        mts = mace_ops.conv_tp_hip(inter, gath[0][:, :, 0], gath.get(1), Y, w)
        return [ops.scatter_edges(flat(mts[l3]), pd).view(-1, 2 * l3 + 1, C)
                .permute(0, 2, 1) for l3 in range(4)]

    def fused():
        m = mace_ops.conv_fused_hip(inter, x, Y, w, pd)
        return [m[l3] for l3 in range(4)]

    def both(fn):
        torch.autograd.grad(fn(), leaves, [G[l3] for l3 in range(4)])

    out = {"N": N, "E": E, "C": C, "P": P, "R": R}
    for name, fn in (("split", split), ("fused", fused)):
        with torch.no_grad():
            f_ms = _median_ms(fn, reps)
        out[name] = {"fwd_ms": f_ms,
                     "fwd_bwd_ms": _median_ms(lambda: both(fn), reps)}
    out["speedup_fwd_bwd"] = (out["split"]["fwd_bwd_ms"]
                              / out["fused"]["fwd_bwd_ms"])

    # the three kernels alone
    K = mace_ops._conv_K(tuple(inter.paths), str(dev))
    xs, Gm = rnd(N, R, C), rnd(N, 16, C)
    Yd, wd = Y.detach(), w.detach()
    M, dxs, dw = torch.empty_like(Gm), torch.empty_like(xs), \
        torch.empty_like(wd)
    dYp = torch.empty(C // 64, E, 16, device=dev)
    kern = {
        "fwd": (lambda: lib.dm_mace_conv_fwd_f32(
            _fp(xs), _fp(wd), _fp(Yd), _fp(K), _ip(pd.src), _ip(pd.row_ptr),
            _fp(M), N, C, layer, _stream()),
            E * (P * C + 16) * 4 + N * (R + 16) * C * 4),
        "bwd_edge": (lambda: lib.dm_mace_conv_bwd_edge_f32(
            _fp(Gm), _fp(xs), _fp(wd), _fp(Yd), _fp(K), _ip(pd.src),
            _ip(pd.row_ptr), _fp(dw), _fp(dYp), N, E, C, layer, _stream()),
            E * (2 * P * C + 16 + 16 * C // 64) * 4
            + N * (R + 16) * C * 4),
        "bwd_node": (lambda: lib.dm_mace_conv_bwd_node_f32(
            _fp(Gm), _fp(wd), _fp(Yd), _fp(K), _ip(pd.dst), _ip(pd.src_perm),
            _ip(pd.src_row_ptr), _fp(dxs), N, C, layer, _stream()),
            E * (P * C + 16) * 4 + N * (R + 16) * C * 4)}
    for name, (fn, nbytes) in kern.items():
        assert fn() == 0, name
        ms = _median_ms(fn, reps)
        out["fused"][name] = {
            "ms": ms, "bytes": nbytes, "TB_per_s": nbytes / ms * 1e-9,
            "share_of_copy_ceiling": nbytes / (ms * 1e-3) / COPY_CEILING}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/mace_conv_standalone.json")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP GPU"
    dev = torch.device("cuda:0")
    from distmlip_amd import gpu_graph
    from distmlip_amd.mace_model import MACEConfig, MACECore
    from distmlip_amd.structures import workload

    s = workload("mace62k", n_gpus=1)
    cfg = MACEConfig(n_elements=int(s.species.max()) + 1, channels=C)
    core = MACECore.seeded(cfg, seed=0)
    pd = gpu_graph.build(s, cfg.r_max, 0.0, 1e-8, False, dev)
    res = {"workload": "mace62k", "copy_ceiling_TB_per_s": 6.29,
           "timer": "HIP events, median of %d" % a.reps}
    for layer in (0, 1):
        res["layer%d" % layer] = _layer_ab(layer, core.interactions[layer],
                                           pd, dev, a.reps)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
