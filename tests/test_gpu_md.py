"""MD integrator kernels (dm_md_kick_drift_f64 / dm_md_kick_reduce_f64) and
the driver's HIP path on the GPU.

The reference of the kernel tests is the fp64 torch composition of
distmlip_amd/md_ops.py on the same device.  Bounds (derived, not tuned):
  vel    4 ulp of the largest term of its sum (ulp(x) <= 2^-52 |x|)
  frac   4 * 2^-52 (values in [0,1)), on the circle for periodic dims; an
         open dim is not wrapped and may exceed 1, where the same 4 ulp are
         4 * 2^-52 * |f|
  sums   N * 2^-53 * sum |terms|   (any summation order of N terms)
  max    exactly equal
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from md_sources import (MASS_SI, TRICLINIC, EinsteinCrystal,  # noqa: E402
                        check_exact_verlet, check_wrap_table, einstein_setup,
                        wrap_table)

from distmlip_amd import md_ops  # noqa: E402
from distmlip_amd.md import ACC, MolecularDynamics  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
SIZES = [1, 63, 64, 65, 255, 256, 257, 70001]
LINV = np.linalg.inv(TRICLINIC)


def _inputs(N, seed, fdtype=torch.float32):
    g = torch.Generator().manual_seed(seed)

    def r(*shape):
        return torch.rand(*shape, dtype=torch.float64, generator=g)

    def n(*shape):
        return torch.randn(*shape, dtype=torch.float64, generator=g)

    frac = r(N, 3)
    # one atom next to three faces so that the smallest case wraps too
    frac[0] = torch.tensor([1e-6, 1.0 - 1e-6, 0.5])
    vel = 0.05 * n(N, 3)
    vel[0] = torch.tensor([-0.05, 0.05, 0.01])
    d = dict(frac=frac, vel=vel, force=n(N, 3).to(fdtype),
             inv_mass=1.0 / (1.0 + 199.0 * r(N)), xi=n(N, 3))
    return {k: v.cuda().contiguous() for k, v in d.items()}


def _circle(d):
    d = d.abs()
    return torch.minimum(d, (1.0 - d).abs())


@pytest.mark.parametrize("N", SIZES)
def test_kick_drift_matches_composition(N):
    a, b, h, c1, c2 = 0.9975, 0.5 * ACC, 1.0, 0.99, 0.0153
    wrapped = 0
    for case, (langevin, masses, pbc, fdtype) in enumerate(
            (lv, m, p, fd) for lv in (False, True) for m in (True, False)
            for p in ((1, 1, 1), (1, 0, 1))
            for fd in (torch.float32, torch.float64)):
        x = _inputs(N, 100 * N + case, fdtype)
        im = x["inv_mass"] if masses else None
        xi = x["xi"] if langevin else None
        fr_r, v_r = x["frac"].clone(), x["vel"].clone()
        fr_k, v_k = x["frac"].clone(), x["vel"].clone()
        md_ops.kick_drift_torch(fr_r, v_r, x["force"], im, a, b, h, LINV, pbc,
                                xi=xi, c1=c1, c2=c2)
        md_ops.kick_drift_hip(fr_k, v_k, x["force"], im, a, b, h, LINV, pbc,
                              xi=xi, c1=c1, c2=c2)
        # largest term of the velocity sum
        t = (im * b).unsqueeze(1) if masses else b
        v1 = x["vel"] * a + x["force"].double() * t
        big = torch.maximum((x["vel"] * a).abs(),
                            (x["force"].double() * t).abs())
        if langevin:
            s = (torch.sqrt(im) * c2).unsqueeze(1) if masses else c2
            big = torch.maximum(big, torch.maximum((v1 * c1).abs(),
                                                   (x["xi"] * s).abs()))
        assert ((v_k - v_r).abs() <= 4 * EPS * big).all(), (case, "vel")
        for k in range(3):
            dk = fr_k[:, k] - fr_r[:, k]
            if pbc[k]:
                assert (_circle(dk) <= 4 * EPS).all(), (case, "frac", k)
                assert ((fr_k[:, k] >= 0) & (fr_k[:, k] < 1)).all()
            else:
                lim = 4 * EPS * fr_r[:, k].abs().clamp(min=1.0)
                assert (dk.abs() <= lim).all(), (case, "frac open", k)
        wrapped += int(((fr_k - x["frac"]).abs() > 0.5).sum())
    assert wrapped >= 1


@pytest.mark.parametrize("N", SIZES)
def test_kick_reduce_matches_composition(N):
    for case, (b, masses, fdtype) in enumerate(
            (b, m, fd) for b in (0.0, 0.5 * ACC) for m in (True, False)
            for fd in (torch.float32, torch.float64)):
        x = _inputs(N, 200 * N + case, fdtype)
        im = x["inv_mass"] if masses else None
        v_r, v_k = x["vel"].clone(), x["vel"].clone()
        red_r = md_ops.kick_reduce_torch(v_r, x["force"], im, b)
        red_k = md_ops.kick_reduce_hip(v_k, x["force"], im, b)
        F = x["force"].double()
        t = (im * b).unsqueeze(1) if masses else b
        big = torch.maximum(x["vel"].abs(), (F * t).abs())
        assert ((v_k - v_r).abs() <= 4 * EPS * big).all(), (case, "vel")
        if b == 0.0:
            assert torch.equal(v_k, x["vel"])
        # per-atom terms of the four sums, from the reference velocities
        v2 = (v_r * v_r).sum(1)
        terms = [v2 / im if masses else v2, (F * v_r).sum(1),
                 (F * F).sum(1), v2]
        for q, term in enumerate(terms):
            lim = N * 2.0 ** -53 * float(term.abs().sum())
            err = abs(float(red_k[q]) - float(red_r[q]))
            assert err <= lim, (case, q, err, lim)
        assert float(red_k[4]) == float(red_r[4]), (case, "max")


def test_wrap_table_kernel():
    periodic, open_ = wrap_table(md_ops.kick_drift_hip, "cuda")
    check_wrap_table(periodic, open_)


def test_bitwise_determinism():
    N = 70001
    x = _inputs(N, 7)
    outs = []
    for _ in range(2):
        fr, v = x["frac"].clone(), x["vel"].clone()
        md_ops.kick_drift_hip(fr, v, x["force"], x["inv_mass"], 0.9975,
                              0.5 * ACC, 1.0, LINV, (1, 1, 1), xi=x["xi"],
                              c1=0.99, c2=0.0153)
        red = md_ops.kick_reduce_hip(v, x["force"], x["inv_mass"], 0.5 * ACC)
        red0 = md_ops.kick_reduce_hip(v, x["force"], None, 0.0)
        outs.append((fr, v, red, red0))
    for p, q in zip(*outs):
        assert torch.equal(p, q)
    assert torch.isfinite(outs[0][2]).all()


def test_rejects_host_and_fp32_state():
    x = _inputs(8, 3)
    with pytest.raises(RuntimeError):
        md_ops.kick_reduce_hip(x["vel"].cpu(), x["force"].cpu(), None, 0.0)
    with pytest.raises(ValueError):
        md_ops.kick_reduce_hip(x["vel"].float(), x["force"], None, 0.0)


def test_verlet_exact_discrete_solution_hip(monkeypatch):
    """The harmonic source evaluated on the device in fp64, the driver on the
    HIP ops (the composition is disabled, so nothing else can have run)."""
    def boom(*a, **k):
        raise AssertionError("torch composition used on a cuda state")
    monkeypatch.setattr(md_ops, "kick_drift_torch", boom)
    monkeypatch.setattr(md_ops, "kick_reduce_torch", boom)
    site, d0, s = einstein_setup()
    src = EinsteinCrystal(site, s.lattice, device="cuda")
    md = MolecularDynamics(s, src, MASS_SI, ensemble="nve", timestep=1.0,
                           loginterval=1000)
    assert md.state.frac.device.type == "cuda"
    worst, wraps = check_exact_verlet(md, src, d0, 1.0, 400)
    print(f"max |d - d0 cos(n theta)| = {worst:.3e} A, {wraps} wraps")
    assert wraps >= 1
    assert worst < 1e-11


def test_nve_on_engine_hip_vs_composition(monkeypatch):
    """10 NVE steps of the fp32 CHGNet engine from 300 K, integrated once by
    the HIP ops and once by the torch composition.  The HIP run's energy
    error is at most 3x the composition run's (their forces diverge in the
    last bits) plus 8 * 2^-24 |E_pot|, the resolution of the engine's fp32
    energy."""
    from distmlip_amd.model import CHGNetCore
    from distmlip_amd.runtime import SpmdEngine
    from distmlip_amd.structures import diamond_si

    eng = SpmdEngine(CHGNetCore.seeded(0), world=1)
    s = diamond_si((4, 2, 2))
    assert s.num_atoms == 128

    def run():
        md = MolecularDynamics(s, eng, MASS_SI, ensemble="nve", timestep=1.0)
        md.state.set_maxwell_boltzmann(300.0, seed=0)
        md.run(10)
        tot = np.array(md.traj.total)
        return float(np.abs(tot - tot[0]).max()), abs(md.traj.potential[0])

    drift_hip, epot = run()
    monkeypatch.setattr(md_ops, "kick_drift", md_ops.kick_drift_torch)
    monkeypatch.setattr(md_ops, "kick_reduce", md_ops.kick_reduce_torch)
    drift_ref, _ = run()
    floor = 8 * 2.0 ** -24 * epot
    print(f"max |E_tot - E_tot(0)| over 10 fs: HIP {drift_hip:.3e} eV, "
          f"composition {drift_ref:.3e} eV, |E_pot| {epot:.4f} eV, "
          f"floor {floor:.3e} eV")
    assert drift_hip <= 3.0 * drift_ref + floor
