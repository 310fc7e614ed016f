"""Microbench (not a test): the fused bf16-MFMA SO(2) convolution against the
path it replaces (so2_conv_split under bf16 autocast and its autograd
reverse), at the uma250k chunk shape: E = 1.5M edges, C = 128.  HIP-event
medians of 5 timed launches per round, 3 rounds alternating between the two
paths; the spread is min..max over all timed launches.  Flop and byte counts
are counted from the shapes (csrc/so2.hip header), not measured.  Run on a GPU:
    python tests/perf_so2_conv.py [out.json] [E]
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C = 128
HBM = 6.29e12          # achievable bytes/s, the figure of the kernel headers
MFMA_BF16 = 2.5e15     # dense bf16 peak flop/s (data sheet), an upper bound
FLOP_EDGE = 2 * 768 * 384 + 4 * 2 * 512 * 256 + 4 * 2 * 256 * 128
BYTES_FWD = 3 * 9 * C * 4            # xs, xd in, mt out
BYTES_BWD = 6 * 9 * C * 4            # go twice, xs, xd in, dxs, dxd out


def timed(fn, n=5):
    ts = []
    for _ in range(n):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return ts


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 3),
            "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3)}


def main():
    from distmlip_amd import uma_ops
    from distmlip_amd.uma_model import UMAConfig, UMACore
    dev = torch.device("cuda:0")
    E = int(sys.argv[2]) if len(sys.argv) > 2 else 1_500_000
    torch.manual_seed(0)
    core = UMACore.seeded(UMAConfig(n_elements=3, sphere_channels=C), seed=0)
    conv = core.blocks[0].msg.float().to(dev).requires_grad_(False)
    xs = torch.randn(E, 9, C, device=dev).requires_grad_(True)
    xd = torch.randn(E, 9, C, device=dev).requires_grad_(True)
    gate = torch.rand(E, 3, device=dev).requires_grad_(True)
    go = torch.randn(E, 9, C, device=dev)
    # the engine hands the split path a bf16 gate (sigmoid under autocast)
    gate_b = gate.detach().bfloat16().requires_grad_(True)

    def fused():
        return uma_ops.so2_conv_fused(conv, xs, xd, gate)

    def split():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return uma_ops.so2_conv_split(conv, xs, xd, gate_b, C).float()

    runs = {"fused_fwd": [], "fused_bwd": [], "split_fwd": [],
            "split_bwd": []}
    for rnd in range(4):                 # round 0 warms up
        for name, fn, g in (("fused", fused, gate), ("split", split, gate_b)):
            out = fn()
            tf = timed(fn)
            tb = timed(lambda: torch.autograd.grad(
                out, (xs, xd, g), go, retain_graph=True))
            del out
            if rnd:
                runs[name + "_fwd"] += tf
                runs[name + "_bwd"] += tb
    r = {"E": E, "C": C, "flop_per_edge": FLOP_EDGE,
         "bytes_per_edge_fwd": BYTES_FWD, "bytes_per_edge_bwd": BYTES_BWD,
         "floor_ms_hbm_fwd": round(E * BYTES_FWD / HBM * 1e3, 3),
         "floor_ms_hbm_bwd": round(E * BYTES_BWD / HBM * 1e3, 3),
         "floor_ms_mfma": round(E * FLOP_EDGE / MFMA_BF16 * 1e3, 3)}
    for k, ts in runs.items():
        r[k] = stats(ts)
    for d, nbytes in (("fwd", BYTES_FWD), ("bwd", BYTES_BWD)):
        sec = r[f"fused_{d}"]["median_ms"] * 1e-3
        r[f"fused_{d}_tflops"] = round(E * FLOP_EDGE / sec / 1e12, 1)
        r[f"fused_{d}_tbytes_s"] = round(E * nbytes / sec / 1e12, 3)
        r[f"fused_{d}_frac_hbm"] = round(E * nbytes / sec / HBM, 3)
        r[f"fused_{d}_frac_mfma"] = round(E * FLOP_EDGE / sec / MFMA_BF16, 3)
        r[f"nearer_bound_{d}"] = "hbm" if r[f"fused_{d}_frac_hbm"] > \
            r[f"fused_{d}_frac_mfma"] else "mfma"
        r[f"speedup_{d}"] = round(r[f"split_{d}"]["median_ms"] /
                                  r[f"fused_{d}"]["median_ms"], 2)
    print(json.dumps(r), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
