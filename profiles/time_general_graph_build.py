"""Timing of the general-lattice GPU graph build against the native CPU
builder on the same input, same process (the numbers quoted in DESIGN.md
and the README "graph build" row).

    python profiles/time_general_graph_build.py --out FILE.json [--big]

Workload: bcc_li(37) (101,306 atoms) with the shear of the test-suite's
`shear_si` applied to its lattice, P=1, bond graph on, cutoff 6.0 / bond
cutoff 3.0.  --big adds diamond_si(50) sheared (1M atoms).  Each figure is
the median of REPS repetitions after WARMUP, device-synchronized around
every repetition.  The unsheared cell through the diagonal fast path is
timed alongside for scale."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distmlip_amd import gpu_graph                      # noqa: E402
from distmlip_amd.dist import Distributed               # noqa: E402
from distmlip_amd.structures import Structure, bcc_li, diamond_si  # noqa: E402

CUTOFF, BOND, TOL = 6.0, 3.0, 1e-8
SHEAR = np.eye(3) + np.array([[0, .08, .05], [0, 0, .1], [0, 0, 0]])
WARMUP, REPS = 2, 7


def sheared(s):
    return Structure(s.frac_coords, s.lattice @ SHEAR, s.species, s.pbc)


def timed(fn, reps=REPS, warmup=WARMUP):
    out = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(out), "min_ms": min(out),
            "max_ms": max(out), "reps": reps}


def measure(name, s, threads, cpu_reps):
    dev = torch.device("cuda:0")
    g = sheared(s)
    assert gpu_graph.fast_scope(s.lattice, s.pbc, CUTOFF)
    assert not gpu_graph.fast_scope(g.lattice, g.pbc, CUTOFF)
    assert gpu_graph.supported(g, CUTOFF)
    nc, R, _, _ = gpu_graph.cell_plan(g.lattice, g.pbc, g.frac_coords,
                                      CUTOFF, TOL)
    pd = gpu_graph.build(g, CUTOFF, BOND, TOL, True, dev)
    rec = {"workload": name, "n_atoms": int(g.num_atoms),
           "n_edges": int(pd.src.numel()), "n_bonds": int(pd.n_bonds),
           "nc": [int(x) for x in nc], "R": [int(x) for x in R],
           "cpu_threads": threads}
    del pd
    rec["gpu_general_sheared"] = timed(
        lambda: gpu_graph.build(g, CUTOFF, BOND, TOL, True, dev))
    rec["gpu_general_sheared_with_guard"] = timed(
        lambda: gpu_graph.supported(g, CUTOFF)
        and gpu_graph.build(g, CUTOFF, BOND, TOL, True, dev))
    rec["gpu_fast_diagonal"] = timed(
        lambda: gpu_graph.build(s, CUTOFF, BOND, TOL, True, dev))
    rec["cpu_native_sheared"] = timed(
        lambda: Distributed.create_distributed(
            g.cart_coords, g.frac_coords, g.lattice, 1, g.pbc, CUTOFF, BOND,
            use_bond_graph=True, num_threads=threads),
        reps=cpu_reps, warmup=1)
    rec["cpu_over_gpu"] = (rec["cpu_native_sheared"]["median_ms"]
                           / rec["gpu_general_sheared_with_guard"]["median_ms"])
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    recs = [measure("bcc_li(37) sheared", bcc_li(37, jitter=0.1, seed=0),
                    a.threads, cpu_reps=5)]
    if a.big:
        recs.append(measure("diamond_si(50) sheared",
                            diamond_si(50, jitter=0.1, seed=0), a.threads,
                            cpu_reps=5))
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0),
                   "results": recs}, f, indent=1)


if __name__ == "__main__":
    main()
