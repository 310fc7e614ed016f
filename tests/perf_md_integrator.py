"""Microbench (not a test): what the MD driver's integrator costs.
Run on a GPU box:
    python tests/perf_md_integrator.py [--out profiles/md_integrator.json]

1. The integrator portion alone, with a zero-force source, at N = 101,306 and
   N = 1,000,000: kick_drift + the D2H copy of frac + kick_reduce, as
     hip    the HIP kernels (distmlip_amd/md_ops.py),
     torch  the fp64 torch composition on the device,
     numpy  a plain numpy version on the host (no D2H: frac is there),
   synchronised host medians of 20 after warm-up, in one process, plus the
   two kernels alone by device events with their algorithmic bytes over time
   (kick_drift 116 B/atom, kick_reduce with the kick 68 B/atom).
2. End to end: 20 NVE steps of the li100k workload through MolecularDynamics
   against bare engine.step on the same structure in the same process, and
   the driver's share of the step.
3. Energy conservation at that size: max |E_tot(t) - E_tot(0)| over 20 fs of
   NVE at dt = 1.0 and dt = 0.5 fs from the same start, on li100k and on
   diamond Si of the same size (23^3 cells, 97,336 atoms); a second-order
   integrator on a smooth energy surface gives a ratio near 4.

GEMM tuning is off (DM_NO_TUNABLEOP=1, as in the test suite): the moving
structure changes the edge count and with it the GEMM shapes every step, and
tuning each new shape costs seconds; the bare engine.step loop runs under the
same setting.  Nothing is asserted; DESIGN.md quotes the output.
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("DM_NO_TUNABLEOP", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distmlip_amd import md_ops  # noqa: E402
from distmlip_amd.md import ACC, MDState, MolecularDynamics  # noqa: E402
from distmlip_amd.structures import bcc_li, diamond_si, workload  # noqa: E402

REPS = 20
MASS = 6.94


def _host_median_ms(fn, reps=REPS, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def _event_median_ms(fn, reps=REPS, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)


def _numpy_step(frac, vel, F, inv_mass, half, dt, linv):
    vel += (half * inv_mass)[:, None] * F
    f = frac + (dt * vel) @ linv
    f -= np.floor(f)
    f[f >= 1.0] = 0.0
    frac[:] = f
    vel += (half * inv_mass)[:, None] * F
    f2 = (F * F).sum(1)
    return ((vel * vel).sum(1) / inv_mass).sum(), (F * vel).sum(), f2.sum(), \
        (vel * vel).sum(), f2.max()


def _say(msg):
    print(f"[perf_md] {msg}", flush=True)


def integrator_alone(structure):
    N = structure.num_atoms
    _say(f"integrator alone, N = {N}")
    st = MDState(structure, MASS, device="cuda")
    st.set_maxwell_boltzmann(300.0, seed=0)
    F = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
    half, dt = 0.5 * ACC, 1.0

    def portion(kd, kr):
        def fn():
            kd(st.frac, st.vel, F, st.inv_mass, 1.0, half, dt, st.linv, st.pbc)
            st.frac.cpu()
            kr(st.vel, F, st.inv_mass, half)
        return fn

    out = {"N": N}
    out["hip_ms"] = _host_median_ms(
        portion(md_ops.kick_drift_hip, md_ops.kick_reduce_hip))
    _say(f"  hip {out['hip_ms']:.3f} ms")
    out["torch_ms"] = _host_median_ms(
        portion(md_ops.kick_drift_torch, md_ops.kick_reduce_torch))
    out["d2h_ms"] = _host_median_ms(lambda: st.frac.cpu())
    _say(f"  torch {out['torch_ms']:.3f} ms, d2h {out['d2h_ms']:.3f} ms")
    hf, hv = st.frac.cpu().numpy().copy(), st.vel.cpu().numpy().copy()
    hF = np.zeros((N, 3))
    him = st.inv_mass.cpu().numpy()
    out["numpy_ms"] = _host_median_ms(
        lambda: _numpy_step(hf, hv, hF, him, half, dt, st.linv))
    _say(f"  numpy {out['numpy_ms']:.3f} ms")
    kd = _event_median_ms(lambda: md_ops.kick_drift_hip(
        st.frac, st.vel, F, st.inv_mass, 1.0, half, dt, st.linv, st.pbc))
    kr = _event_median_ms(lambda: md_ops.kick_reduce_hip(
        st.vel, F, st.inv_mass, half))
    out["kick_drift_ms"], out["kick_reduce_ms"] = kd, kr
    out["kick_drift_TBps"] = 116.0 * N / (kd * 1e-3) / 1e12
    out["kick_reduce_TBps"] = 68.0 * N / (kr * 1e-3) / 1e12
    out["fastest"] = min(("hip", "torch", "numpy"),
                         key=lambda k: out[k + "_ms"])
    return out


def end_to_end(nsteps=20):
    from distmlip_amd.model import CHGNetCore
    from distmlip_amd.runtime import SpmdEngine
    s = workload("li100k")
    eng = SpmdEngine(CHGNetCore.seeded(0), world=1)
    _say(f"end to end, N = {s.num_atoms}: bare engine.step")
    for _ in range(3):
        eng.step(s)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(nsteps):
        eng.step(s)
    torch.cuda.synchronize()
    bare = (time.perf_counter() - t0) * 1e3 / nsteps
    md = MolecularDynamics(s, eng, MASS, ensemble="nve", timestep=1.0,
                           loginterval=nsteps)
    md.state.set_maxwell_boltzmann(300.0, seed=0)
    _say(f"  engine.step {bare:.2f} ms; MolecularDynamics")
    md.run(3)
    torch.cuda.synchronize()
    _say("  warm-up done")
    t0 = time.perf_counter()
    md.run(nsteps)
    torch.cuda.synchronize()
    drv = (time.perf_counter() - t0) * 1e3 / nsteps
    tot = md.traj.total
    return {"N": s.num_atoms, "steps": nsteps, "engine_step_ms": bare,
            "md_step_ms": drv, "driver_share": (drv - bare) / drv,
            "etot_first_last": [tot[0], tot[-1]]}


def energy_order(s, mass, eng):
    out = {"N": s.num_atoms, "span_fs": 20.0, "mass": mass}
    for dt in (1.0, 0.5):
        md = MolecularDynamics(s, eng, mass, ensemble="nve", timestep=dt)
        md.state.set_maxwell_boltzmann(300.0, seed=0)
        md.run(int(round(20.0 / dt)))
        tot = np.array(md.traj.total)
        key = f"dt_{dt}"
        out[key] = {"max_abs_dE": float(np.abs(tot - tot[0]).max()),
                    "total": tot.tolist(), "kinetic": md.traj.kinetic,
                    "temperature": md.traj.temperature}
        _say(f"energy, dt = {dt}: max |dE_tot| {out[key]['max_abs_dE']:.4f} eV"
             f" on E_kin(0) {md.traj.kinetic[0]:.1f} eV, T {md.traj.temperature[0]:.1f}"
             f" -> {md.traj.temperature[-1]:.1f} K")
    out["ratio"] = out["dt_1.0"]["max_abs_dE"] / out["dt_0.5"]["max_abs_dE"]
    _say(f"  ratio {out['ratio']:.3f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/md_integrator.json")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-integrator", action="store_true")
    ap.add_argument("--skip-energy", action="store_true")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS}
    if os.path.exists(args.out):        # the two parts may run separately
        with open(args.out) as fh:
            res.update(json.load(fh))
    if not args.skip_integrator:
        res["integrator"] = [integrator_alone(bcc_li(37, jitter=0.1)),
                             integrator_alone(diamond_si(50, jitter=0.1))]
    if not args.skip_e2e:
        res["end_to_end_li100k"] = end_to_end()
    if not args.skip_energy:
        from distmlip_amd.model import CHGNetCore
        from distmlip_amd.runtime import SpmdEngine
        eng = SpmdEngine(CHGNetCore.seeded(0), world=1)
        _say("energy: li100k")
        res["energy_li100k"] = energy_order(workload("li100k"), MASS, eng)
        _say("energy: diamond_si(23)")
        res["energy_si97k"] = energy_order(diamond_si(23, jitter=0.1),
                                           28.0855, eng)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
