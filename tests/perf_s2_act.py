"""Microbench (not a test): the fused fp32-MFMA S2 grid activation against the
torch composition it replaces (uma_ops.s2_act with DM_UMA_S2=torch: chunks of
65 536 nodes, checkpointed reverse), in fp32 and under bf16 autocast, at
N = 65 536 (one chunk) and N = 238 000, C = 128, G = 16 x 32 = 512.
HIP-event medians of 3 timed calls per round, 3 rounds alternating between
the paths; the spread is min..max over all timed calls.  Flop and byte counts
are counted from the shapes, not measured.  Run on a GPU:
    python tests/perf_s2_act.py [out.json]
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C, G = 128, 512
HBM = 6.29e12          # achievable bytes/s, the figure of the kernel headers
MFMA_F32 = 157.3e12    # dense fp32 matrix peak flop/s (data sheet)
VALU_F32 = 256 * 4 * 16 * 2.4e9   # fp32 VALU instructions x lanes per second
# per (node, channel, grid point): algorithm flops (K = 9 both ways), the
# flops the padded MFMAs execute (K = 12, M = 16), VALU instructions of silu
FLOP = {"fwd": 2 * 9 + 2 * 9, "bwd": 3 * 2 * 9}
FLOP_PAD = {"fwd": 2 * 12 + 2 * 16, "bwd": 2 * 2 * 12 + 2 * 16}
VALU = {"fwd": 15, "bwd": 14 + 6}
BYTES = {"fwd": 2 * 9 * 4, "bwd": 3 * 9 * 4}      # per (node, channel)


def timed(fn, n=3):
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


def bench_shape(N):
    from distmlip_amd import uma_ops
    from distmlip_amd.uma_model import UMAConfig
    cfg = UMAConfig(n_elements=3, sphere_channels=C)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x = (2 * torch.randn(N, 9, C, device=dev)).requires_grad_(True)
    xb = x.detach().bfloat16().requires_grad_(True)
    go = torch.randn(N, 9, C, device=dev)

    def path(env, inp):
        def fwd():
            os.environ["DM_UMA_S2"] = env
            return uma_ops.s2_act(inp, cfg)
        return fwd, inp

    paths = {"kernel": path("hip", x), "kernel_bf16in": path("hip", xb),
             "torch_f32": path("torch", x), "torch_bf16": path("torch", xb)}
    runs = {f"{k}_{d}": [] for k in paths for d in ("fwd", "bwd")}
    for rnd in range(4):                 # round 0 warms up
        for name, (fn, inp) in paths.items():
            out = fn()
            tf = timed(fn)
            gout = go.to(out.dtype)
            # the checkpointed reverse recomputes: no retain_graph there
            def bwd():
                o = fn()
                torch.cuda.synchronize()
                s = torch.cuda.Event(enable_timing=True)
                e = torch.cuda.Event(enable_timing=True)
                s.record()
                torch.autograd.grad(o, inp, gout)
                e.record()
                torch.cuda.synchronize()
                return s.elapsed_time(e)
            tb = [bwd() for _ in range(3)]
            del out
            if rnd:
                runs[name + "_fwd"] += tf
                runs[name + "_bwd"] += tb
    r = {"N": N, "C": C, "G": G}
    for k, ts in runs.items():
        r[k] = stats(ts)
    work = N * C * G
    for d in ("fwd", "bwd"):
        sec = r[f"kernel_{d}"]["median_ms"] * 1e-3
        r[f"kernel_{d}_tflops"] = round(work * FLOP[d] / sec / 1e12, 1)
        r[f"kernel_{d}_frac_mfma_padded"] = round(
            work * FLOP_PAD[d] / sec / MFMA_F32, 3)
        r[f"kernel_{d}_frac_valu"] = round(work * VALU[d] / sec / VALU_F32, 3)
        r[f"kernel_{d}_frac_hbm"] = round(N * C * BYTES[d] / sec / HBM, 3)
        fr = {b: r[f"kernel_{d}_frac_{b}"]
              for b in ("mfma_padded", "valu", "hbm")}
        r[f"nearest_bound_{d}"] = max(fr, key=fr.get)
        for ref in ("torch_f32", "torch_bf16"):
            r[f"speedup_{d}_vs_{ref}"] = round(
                r[f"{ref}_{d}"]["median_ms"] / r[f"kernel_{d}"]["median_ms"], 2)
    return r


def main():
    res = [bench_shape(N) for N in (65_536, 238_000)]
    for r in res:
        print(json.dumps(r), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
