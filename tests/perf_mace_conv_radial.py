"""Microbench (not a test): the fused MACE convolution fed by the torch last
radial layer (tp_w = h @ Wr.T, conv_fused_hip) against the kernels that form
tp_w inside (conv_radial_hip), on the graph of the mace62k workload, C = 128.
Run on a GPU box:
    python tests/perf_mace_conv_radial.py \
        [--out profiles/mace_conv_radial_standalone.json]

HIP-event medians.  The new kernels are bound by their fp32 MFMAs: the
forward and bwd_node form w once each, bwd_edge forms w and dh, 2*E*H*P*C
flop apiece, so a layer's three kernels do 4 * 2*E*H*P*C flop, set against
the 157.3 TFLOP/s fp32 matrix peak of the MI355X.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.perf_tn_message import _median_ms  # noqa: E402

C, H = 128, 64
MFMA_F32 = 157.3e12    # dense fp32 matrix peak flop/s (data sheet)


def _layer_ab(layer, inter, pd, dev, reps):
    from distmlip_amd import mace_ops
    from distmlip_amd.ops import _fp, _ip, _stream, hip_lib
    lib = hip_lib()
    N, E, P, R = pd.n_atoms, pd.src.shape[0], len(inter.paths), (1, 4)[layer]
    g = torch.Generator(device=dev).manual_seed(layer)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    x = {l: rnd(N, C, 2 * l + 1).requires_grad_(True)
         for l in range(layer + 1)}
    Y, h = rnd(E, 16).requires_grad_(True), rnd(E, H).requires_grad_(True)
    G = [rnd(N, C, 2 * l3 + 1) for l3 in range(4)]
    leaves = list(x.values()) + [Y, h]
    Wr = inter.radial.layers[-1].weight

    def fused():
        m = mace_ops.conv_fused_hip(inter, x, Y, (h @ Wr.t()).view(E, P, C),
                                    pd)
        return [m[l3] for l3 in range(4)]

    def radial():
        m = mace_ops.conv_radial_hip(inter, x, Y, h, pd)
        return [m[l3] for l3 in range(4)]

    out = {"N": N, "E": E, "C": C, "P": P, "R": R, "H": H}
    for name, fn in (("fused", fused), ("radial", radial)):
        with torch.no_grad():
            f_ms = _median_ms(fn, reps)
        out[name] = {"fwd_ms": f_ms, "fwd_bwd_ms": _median_ms(
            lambda: torch.autograd.grad(fn(), leaves, G), reps)}
    out["speedup_fwd_bwd"] = (out["fused"]["fwd_bwd_ms"]
                              / out["radial"]["fwd_bwd_ms"])

    # the three kernels alone
    K = mace_ops._conv_K(tuple(inter.paths), str(dev))
    Wa, Wb = mace_ops._conv_wr_packed(inter, C)
    xs, Gm = rnd(N, R, C), rnd(N, 16, C)
    Yd, hd = Y.detach(), h.detach()
    M, dxs = torch.empty_like(Gm), torch.empty_like(xs)
    dhp = torch.empty(C // 64, E, H, device=dev)
    dYp = torch.empty(C // 64, E, 16, device=dev)
    gemm = 2 * E * H * P * C
    kern = {
        "fwd": (lambda: lib.dm_mace_conv_rad_fwd_f32(
            _fp(xs), _fp(hd), _fp(Wa), _fp(Yd), _fp(K), _ip(pd.src),
            _ip(pd.row_ptr), _fp(M), N, C, H, layer, _stream()), gemm),
        "bwd_edge": (lambda: lib.dm_mace_conv_rad_bwd_edge_f32(
            _fp(Gm), _fp(xs), _fp(hd), _fp(Wa), _fp(Wb), _fp(Yd), _fp(K),
            _ip(pd.src), _ip(pd.row_ptr), _fp(dhp), _fp(dYp), N, E, C, H,
            layer, _stream()), 2 * gemm),
        "bwd_node": (lambda: lib.dm_mace_conv_rad_bwd_node_f32(
            _fp(Gm), _fp(hd), _fp(Wa), _fp(Yd), _fp(K), _ip(pd.dst),
            _ip(pd.src_perm), _ip(pd.src_row_ptr), _fp(dxs), N, C, H, layer,
            _stream()), gemm)}
    total_ms = 0.0
    for name, (fn, flop) in kern.items():
        assert fn() == 0, name
        ms = _median_ms(fn, reps)
        total_ms += ms
        out["radial"][name] = {
            "ms": ms, "mfma_flop": flop, "TFLOP_per_s": flop / ms * 1e-9,
            "share_of_fp32_matrix_peak": flop / (ms * 1e-3) / MFMA_F32}
    out["radial"]["kernels"] = {
        "ms": total_ms, "mfma_flop": 4 * gemm,
        "TFLOP_per_s": 4 * gemm / total_ms * 1e-9,
        "share_of_fp32_matrix_peak": 4 * gemm / (total_ms * 1e-3) / MFMA_F32}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out",
                    default="profiles/mace_conv_radial_standalone.json")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP GPU"
    dev = torch.device("cuda:0")
    from distmlip_amd import gpu_graph
    from distmlip_amd.mace_model import MACEConfig, MACECore
    from distmlip_amd.structures import workload

    s = workload("mace62k", n_gpus=1)
    cfg = MACEConfig(n_elements=int(s.species.max()) + 1, channels=C)
    core = MACECore.seeded(cfg, seed=0).to(dev).requires_grad_(False)
    pd = gpu_graph.build(s, cfg.r_max, 0.0, 1e-8, False, dev)
    res = {"workload": "mace62k", "fp32_matrix_peak_TFLOP_per_s": 157.3,
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
