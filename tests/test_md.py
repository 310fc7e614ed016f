"""Native MD / relaxation driver (distmlip_amd/md.py) on CPU in fp64:
exact discrete solutions of the integrators, order of accuracy on a real
engine, reversibility, the periodic wrap, thermostats, FIRE and the API."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from md_sources import (MASS_SI, EinsteinCrystal, ZeroForces,  # noqa: E402
                        check_exact_verlet, check_wrap_table, einstein_setup,
                        wrap_table)

from distmlip_amd import gpu_graph, md_ops  # noqa: E402
from distmlip_amd.md import (ACC, KB, MDState, MolecularDynamics,  # noqa: E402
                             Relaxer)
from distmlip_amd.structures import Structure, diamond_si  # noqa: E402


def test_constants():
    # 1 eV/(A amu) in A/fs^2 from the exact SI e and the 2018 amu, to the
    # ten digits the module carries
    assert ACC == pytest.approx(1.602176634e-19 / 1.66053906660e-27 * 1e-10,
                                rel=1e-9)
    assert KB == pytest.approx(1.380649e-23 / 1.602176634e-19, rel=1e-9)


# -- exact discrete solution ---------------------------------------------------

def test_verlet_exact_discrete_solution():
    site, d0, s = einstein_setup()
    src = EinsteinCrystal(site, s.lattice)
    md = MolecularDynamics(s, src, MASS_SI, ensemble="nve", timestep=1.0,
                           loginterval=1000)
    worst, wraps = check_exact_verlet(md, src, d0, 1.0, 400)
    print(f"max |d - d0 cos(n theta)| = {worst:.3e} A, {wraps} wraps")
    assert wraps >= 1
    assert worst < 1e-11


def test_reversibility():
    site, d0, s = einstein_setup(seed=1)
    src = EinsteinCrystal(site, s.lattice)
    md = MolecularDynamics(s, src, MASS_SI, ensemble="nve", timestep=1.0,
                           loginterval=1000)
    md.run(100)
    md.state.vel.neg_()
    md.invalidate()
    md.run(100)
    d = src.displacement(md.state.frac.cpu().numpy()).numpy()
    err = float(np.abs(d - d0).max())
    print(f"return error {err:.3e} A")
    assert err < 1e-10
    assert float(md.state.vel.abs().max()) < 1e-12


# -- a real engine -------------------------------------------------------------

@pytest.fixture(scope="module")
def chgnet_engine():
    from distmlip_amd.model import CHGNetCore
    from distmlip_amd.runtime import SpmdEngine
    from oracle.chgnet_ref import CpuRefOps
    core = CHGNetCore.seeded(0).double()
    return SpmdEngine(core, world=1, threads=2, device="cpu", ops=CpuRefOps())


def _drift(engine, dt, nsteps):
    s = diamond_si((2, 2, 2), jitter=0.05, seed=3)
    md = MolecularDynamics(s, engine, MASS_SI, ensemble="nve", timestep=dt)
    md.state.set_maxwell_boltzmann(300.0, seed=0)
    assert md.state.temperature() == pytest.approx(300.0, rel=1e-12)
    m = 1.0 / md.state.inv_mass
    assert float((m[:, None] * md.state.vel).sum(0).abs().max()) < 1e-12
    traj = md.run(nsteps)
    tot = np.array(traj.total)
    assert len(tot) == nsteps + 1
    return float(np.abs(tot - tot[0]).max())


def test_second_order_energy_error(chgnet_engine):
    d1 = _drift(chgnet_engine, 1.0, 20)
    d2 = _drift(chgnet_engine, 0.5, 40)
    print(f"max |dE_tot| over 20 fs: dt=1.0 {d1:.5f} eV, dt=0.5 {d2:.5f} eV, "
          f"ratio {d1 / d2:.3f}")
    assert 3.0 <= d1 / d2 <= 5.0


# -- wrap table ----------------------------------------------------------------

def test_wrap_table():
    periodic, open_ = wrap_table(md_ops.kick_drift, "cpu")
    check_wrap_table(periodic, open_)


# -- thermostats ---------------------------------------------------------------

def _gas(n, seed=0):
    rng = np.random.default_rng(seed)
    return Structure(frac_coords=rng.random((n, 3)), lattice=np.eye(3) * 30.0,
                     species=np.zeros(n, dtype=np.int64),
                     pbc=np.ones(3, dtype=np.int64))


def test_berendsen_recurrence():
    T0, Ti, dt, taut = 300.0, 600.0, 1.0, 100.0
    md = MolecularDynamics(_gas(200), ZeroForces(), [MASS_SI], ensemble="nvt",
                           temperature=T0, timestep=dt, taut=taut,
                           loginterval=1000)
    md.state.set_maxwell_boltzmann(Ti, seed=1)
    for n in range(1, 51):
        md.step()
        want = T0 + (Ti - T0) * (1.0 - dt / taut) ** n
        assert md.state.temperature() == pytest.approx(want, rel=1e-10), n


def test_berendsen_default_taut():
    md = MolecularDynamics(_gas(8), ZeroForces(), MASS_SI, timestep=2.0)
    assert md.ensemble == "nvt" and md.taut == 200.0


def test_langevin_zero_temperature_decay():
    gamma, dt = 0.02, 1.0
    md = MolecularDynamics(_gas(50), ZeroForces(), MASS_SI,
                           ensemble="nvt_langevin", temperature=0.0,
                           friction=gamma, timestep=dt, loginterval=1000)
    md.state.set_maxwell_boltzmann(500.0, seed=2)
    v0 = md.state.vel.clone()
    for n in range(1, 41):
        md.step()
        want = v0 * math.exp(-gamma * n * dt)
        rel = ((md.state.vel - want).abs() / want.abs()).max().item()
        assert rel < 1e-12, (n, rel)


def _langevin_run(seed, n=20000, steps=200, gamma=0.1):
    md = MolecularDynamics(_gas(n), ZeroForces(), MASS_SI,
                           ensemble="nvt_langevin", temperature=300.0,
                           friction=gamma, timestep=1.0, seed=seed,
                           loginterval=10 ** 6)
    md.run(steps)
    return md


def test_langevin_temperature_and_seed():
    # 200 fs at friction 0.1/fs = 20/gamma of simulated time; with zero
    # forces the O step is exact for any gamma dt
    a = _langevin_run(seed=5)
    T = a.state.temperature()
    sigma = math.sqrt(2.0 / (3 * 20000))
    print(f"T = {T:.2f} K, 4 sigma = {4 * sigma * 300:.2f} K")
    assert abs(T / 300.0 - 1.0) < 0.024
    assert 4 * sigma < 0.024
    b = _langevin_run(seed=5, n=2000, steps=20)
    c = _langevin_run(seed=5, n=2000, steps=20)
    d = _langevin_run(seed=6, n=2000, steps=20)
    assert torch.equal(b.state.vel, c.state.vel)
    assert torch.equal(b.state.frac, c.state.frac)
    assert not torch.equal(b.state.vel, d.state.vel)


# -- FIRE ----------------------------------------------------------------------

def test_fire_harmonic():
    site, d0, s = einstein_setup(seed=2)
    src = EinsteinCrystal(site, s.lattice)
    out = Relaxer(src).relax(s, fmax=1e-6, steps=200)
    print(f"FIRE: {out['nsteps']} iterations, fmax {out['fmax']:.2e}")
    assert out["converged"] and out["nsteps"] <= 200
    assert out["fmax"] < 1e-6
    d = src.displacement(out["final_structure"].frac_coords).numpy()
    assert np.abs(d).max() < 1e-6 / 2.0 * 1.01
    assert len(out["trajectory"]) == out["nsteps"] + 1


def test_fire_chgnet(chgnet_engine, tmp_path):
    s = diamond_si((2, 2, 2), jitter=0.05, seed=3)
    path = str(tmp_path / "relax.npz")
    out = Relaxer(chgnet_engine).relax(s, fmax=0.05, steps=30,
                                       traj_file=path, interval=5)
    E = out["trajectory"].potential
    print(f"FIRE on CHGNet: E {E[0]:.6f} -> {E[-1]:.6f} eV in "
          f"{out['nsteps']} iterations, fmax {out['fmax']:.4f}")
    assert E[-1] < E[0]
    assert gpu_graph.supported(out["final_structure"], 6.0)
    z = np.load(path)
    assert z["frac"].shape[1:] == (64, 3)
    assert list(z["step"][:2]) == [0, 5]


# -- API -----------------------------------------------------------------------

def test_unsupported_ensemble_lists_supported():
    for name in ("npt", "nvt_andersen", "nvt_bussi", "nvt_nose_hoover",
                 "npt_berendsen", "npt_nose_hoover", "bogus"):
        with pytest.raises(ValueError) as e:
            MolecularDynamics(_gas(4), ZeroForces(), MASS_SI, ensemble=name)
        for ok in ("nve", "nvt", "nvt_langevin"):
            assert repr(ok) in str(e.value)


def test_relax_cell_raises():
    with pytest.raises(NotImplementedError):
        Relaxer(ZeroForces()).relax(_gas(4), relax_cell=True)


def test_masses_forms():
    s = _gas(6)
    s.species = np.array([0, 1, 0, 1, 1, 0])
    per_atom = MDState(s, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    assert (1.0 / per_atom.inv_mass).tolist() == [1, 2, 3, 4, 5, 6]
    table = MDState(s, [10.0, 20.0])
    assert (1.0 / table.inv_mass).tolist() == [10, 20, 10, 20, 20, 10]
    assert torch.equal(MDState(s, {0: 10.0, 1: 20.0}).inv_mass, table.inv_mass)
    with pytest.raises(ValueError):
        MDState(s, None)
    with pytest.raises(ValueError):
        MDState(s, [10.0])            # no mass for species 1


def test_non_finite_kinetic_energy_names_step():
    class Blowup(ZeroForces):
        def forces(self, structure):
            E, F = super().forces(structure)
            self.n = getattr(self, "n", 0) + 1
            if self.n == 3:                       # the forces of step 2
                F[0, 0] = float("inf")
            return E, F
    md = MolecularDynamics(_gas(4), Blowup(), MASS_SI, ensemble="nve")
    with pytest.raises(FloatingPointError, match="step 2"):
        md.run(5)


def test_trajectory_and_log(tmp_path):
    site, d0, s = einstein_setup(seed=4, n=16)
    src = EinsteinCrystal(site, s.lattice)
    log, traj = str(tmp_path / "md.log"), str(tmp_path / "md.npz")
    md = MolecularDynamics(s, src, MASS_SI, ensemble="nve", logfile=log,
                           loginterval=5, trajectory=traj)
    md.run(20)
    md.close()
    z = np.load(traj)
    assert z["step"].tolist() == [0, 5, 10, 15, 20]
    assert z["frac"].shape == (5, 16, 3)
    assert ((z["frac"] >= 0) & (z["frac"] < 1)).all()
    np.testing.assert_allclose(z["total"], z["potential"] + z["kinetic"])
    assert np.abs(z["total"] - z["total"][0]).max() < 1e-3 * z["total"][0]
    assert z["temperature"][0] == 0.0 and z["temperature"][1] > 0
    assert len(open(log).read().strip().splitlines()) == 6
    assert src.calls == 21            # one forces() per step plus the first


def test_potential_dist_matches_engine(core64, si_slab):
    from distmlip_amd.chgnet import CHGNet_Dist
    from distmlip_amd.pes import Potential_Dist
    from distmlip_amd.runtime import SpmdEngine
    from oracle.chgnet_ref import CpuRefOps

    model = CHGNet_Dist.from_existing(core64, dtype=torch.float64)
    model.enable_distributed_mode(["cpu"] * 2,
                                  ops_factory=lambda dev: CpuRefOps())
    pot = Potential_Dist(model, calc_forces=True)
    eng = SpmdEngine(core64, world=1, threads=2, device="cpu",
                     ops=CpuRefOps())
    fracs = []
    for calc in (pot, eng):
        md = MolecularDynamics(si_slab, calc, [MASS_SI], ensemble="nve",
                               timestep=1.0)
        md.state.set_maxwell_boltzmann(300.0, seed=0)
        md.run(3)
        fracs.append(md.state.frac.numpy().copy())
    df = fracs[0] - fracs[1]
    df -= np.round(df)
    err = float(np.abs(df @ si_slab.lattice).max())
    print(f"Potential_Dist vs engine after 3 steps: {err:.3e} A")
    assert err < 1e-9


# -- launches and reads per step -----------------------------------------------

class _Watched:
    """Stands in for kick_reduce's result: notes every read of it."""

    def __init__(self, red, log):
        self._red, self._log = red, log

    def __getitem__(self, i):
        self._log.append("read")
        return self._red[i]

    def tolist(self):
        self._log.append("read")
        return self._red.tolist()

    def __float__(self):
        raise AssertionError("the [5] result has no scalar value")


@pytest.mark.parametrize("ensemble", ["nve", "nvt_langevin"])
def test_one_reduce_per_step_and_no_reads_between_logs(monkeypatch, ensemble):
    site, d0, s = einstein_setup(seed=5, n=16)
    src = EinsteinCrystal(site, s.lattice)
    md = MolecularDynamics(s, src, MASS_SI, ensemble=ensemble, loginterval=5)
    md.potential_energy                   # first forces() and frame 0
    calls, reads = [], []
    real_reduce, real_drift = md_ops.kick_reduce, md_ops.kick_drift

    def reduce(vel, force, inv_mass, b):
        calls.append("reduce")
        return _Watched(real_reduce(vel, force, inv_mass, b), reads)

    def drift(*a, **k):
        calls.append("drift")
        return real_drift(*a, **k)

    monkeypatch.setattr(md_ops, "kick_reduce", reduce)
    monkeypatch.setattr(md_ops, "kick_drift", drift)
    before = src.calls
    for n in range(1, 11):
        md.step()
        assert calls == ["drift", "reduce"] * n
        assert len(reads) == n // 5       # read on logging steps only
    assert src.calls - before == 10
    assert md.traj.steps == [0, 5, 10]
    # on demand, between logs: one more reduction, then cached
    md.step()
    assert md.kinetic_energy > 0 and md.kinetic_energy > 0
    assert calls.count("reduce") == 12


def test_berendsen_reads_every_step_but_reduces_once(monkeypatch):
    md = MolecularDynamics(_gas(20), ZeroForces(), MASS_SI, ensemble="nvt",
                           loginterval=100)
    md.state.set_maxwell_boltzmann(600.0, seed=1)
    md.potential_energy
    n_red = []
    real = md_ops.kick_reduce
    monkeypatch.setattr(md_ops, "kick_reduce",
                        lambda *a: (n_red.append(1), real(*a))[1])
    md.run(7)
    assert len(n_red) == 7


def test_berendsen_is_not_clipped():
    # lambda^2 = 1 + 0.5 (300/10 - 1) = 15.5: far outside [0.9, 1.1]^2
    md = MolecularDynamics(_gas(50), ZeroForces(), MASS_SI, ensemble="nvt",
                           temperature=300.0, timestep=1.0, taut=2.0)
    md.state.set_maxwell_boltzmann(10.0, seed=3)
    md.step()
    assert md.state.temperature() == pytest.approx(10.0 + 0.5 * 290.0,
                                                   rel=1e-12)


def test_fire_first_move_keeps_dt():
    """ASE's first FIRE step has no velocity yet: v = dt F with dt = 0.1
    unchanged, so dr = 0.01 F = -0.02 d0 on the k = 2 harmonic source."""
    site, d0, s = einstein_setup(seed=6)
    src = EinsteinCrystal(site, s.lattice)
    out = Relaxer(src).relax(s, fmax=1e-9, steps=1)
    assert out["nsteps"] == 1 and not out["converged"]
    d = src.displacement(out["final_structure"].frac_coords).numpy()
    assert np.abs(d - 0.98 * d0).max() < 1e-13


def test_masses_length_n_is_per_atom():
    s = _gas(2)
    s.species = np.array([1, 0])
    assert (1.0 / MDState(s, [10.0, 20.0]).inv_mass).tolist() == [10, 20]
    assert (1.0 / MDState(s, {0: 10.0, 1: 20.0}).inv_mass).tolist() == [20, 10]


def test_engine_adapter_scopes_gemm_tuning(monkeypatch):
    """New-shape GEMM tuning is off inside the adapter's engine.step() and
    back to the caller's setting afterwards; tune_new_gemm_shapes=True
    leaves it alone."""
    from distmlip_amd.md import EngineForces

    class Tunable:
        enabled, tuning = True, True
        def is_enabled(self): return self.enabled
        def tuning_is_enabled(self): return self.tuning
        def tuning_enable(self, v): self.tuning = bool(v)

    tun = Tunable()
    monkeypatch.setattr(torch.cuda, "tunable", tun, raising=False)

    class Engine:
        device, world = torch.device("cuda"), 1
        seen = []
        def step(self, structure):
            self.seen.append(tun.tuning)
            if len(self.seen) == 3:
                raise RuntimeError("step failed")
            return {"energy": torch.zeros(()),
                    "forces_owned": torch.zeros(4, 3),
                    "global_ids_owned": np.arange(4)}

    eng = Engine()
    EngineForces(eng).forces(_gas(4))
    assert eng.seen == [False] and tun.tuning is True
    EngineForces(eng, tune_new_gemm_shapes=True).forces(_gas(4))
    assert eng.seen == [False, True] and tun.tuning is True
    with pytest.raises(RuntimeError):
        EngineForces(eng).forces(_gas(4))
    assert tun.tuning is True                     # restored after a failure
    tun.tuning = False                            # the caller's own choice
    EngineForces(eng).forces(_gas(4))
    assert tun.tuning is False
