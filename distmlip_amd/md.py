"""Native molecular dynamics and relaxation on top of the engines.

The reference ships `Relaxer` and `MolecularDynamics` as thin wrappers over
ASE (implementations/matgl/ase.py:130-490; mirrored, ASE required, in
distmlip_amd/ase.py).  This module needs no ASE: the integrator state lives
on the engine's device in fp64 and advances through two fused ops
(distmlip_amd/md_ops.py: HIP kernels on a GPU, an fp64 torch composition on
a CPU device).

Per step the driver issues
  1. one `kick_drift`  (half-kick with the previous forces, drift, wrap),
  2. one device-to-host copy of frac into a `Structure` (the engines take a
     host structure),
  3. one `forces()` call,
  4. one `kick_reduce` (second half-kick and the sums of the step).
Scalars are read back (which synchronises the device) only on steps that
log, record or thermostat.

Units: eV, Angstrom, amu, fs, K.  Velocities are A/fs.

Force source protocol: any object with
    forces(structure) -> (energy, F)      # F: [N,3] on the state's device
and an optional `device` attribute.  `EngineForces` adapts the four SPMD
engines (step() -> energy / forces_owned / global_ids_owned),
`PotentialForces` adapts `Potential_Dist`; tests drive the integrators with
analytic sources through the same protocol.

For world > 1 the integrator state is REPLICATED: every rank holds all
atoms, receives identical forces (owned forces scattered into zeros, then
all_reduce(SUM): each atom has one owner, so the sum adds exact zeros) and
performs identical arithmetic, so the ranks stay bit-identical without
exchanging state.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from distmlip_amd import md_ops
from distmlip_amd.structures import Structure

# 1 eV/(A amu) in A/fs^2: e / m_u * 1e-10, with the exact SI
# e = 1.602176634e-19 C.  The ten digits are e * N_A (the Faraday constant,
# m_u = 1 g/mol / N_A); the 2018 CODATA m_u = 1.66053906660e-27 kg gives
# 9.6485332157e-3, 4e-10 relative away, far below any model's force error.
ACC = 9.648533212e-3
KB = 8.617333262e-5            # eV/K

ENSEMBLES = ("nve", "nvt", "nvt_langevin")


# ---------------------------------------------------------------------------
# force sources
# ---------------------------------------------------------------------------

class EngineForces:
    """Force source over SpmdEngine / MaceSpmdEngine / UmaSpmdEngine /
    TensorNetSpmdEngine: scatters `forces_owned` into a zero-filled [N,3]
    by `global_ids_owned`; for world > 1 an all_reduce(SUM) completes it on
    every rank (one owner per atom: the sum adds exact zeros, every rank
    holds identical bits).

    `tune_new_gemm_shapes`: the engines switch on per-shape GEMM tuning for
    a frozen structure.  Under dynamics the edge count, and with it every
    [E,*] GEMM shape, changes from step to step, and tuning a new shape
    costs seconds.  With the default False, tuning of NEW shapes is switched
    off for the duration of each engine.step() this adapter issues (shapes
    already tuned keep their choice) and the process-wide setting is put
    back afterwards; True leaves the setting alone."""

    def __init__(self, engine, tune_new_gemm_shapes: bool = False):
        self.engine = engine
        self.device = torch.device(engine.device)
        self.world = int(getattr(engine, "world", 1))
        self.tune_new_gemm_shapes = bool(tune_new_gemm_shapes)

    def _step(self, structure):
        tunable = getattr(torch.cuda, "tunable", None)
        if self.tune_new_gemm_shapes or self.device.type != "cuda" \
                or tunable is None or not tunable.is_enabled() \
                or not tunable.tuning_is_enabled():
            return self.engine.step(structure)
        tunable.tuning_enable(False)
        try:
            return self.engine.step(structure)
        finally:
            tunable.tuning_enable(True)

    def forces(self, structure):
        out = self._step(structure)
        fo = out["forces_owned"].detach()
        F = torch.zeros((structure.num_atoms, 3), dtype=fo.dtype,
                        device=fo.device)
        gids = torch.as_tensor(np.asarray(out["global_ids_owned"]),
                               dtype=torch.int64, device=fo.device)
        F[gids] = fo
        if self.world > 1:
            import torch.distributed as dist
            dist.all_reduce(F)
        return out["energy"].detach(), F


class PotentialForces:
    """Force source over Potential_Dist (forward -> E, F, stress, hessian)."""

    def __init__(self, potential):
        if not potential.calc_forces:
            raise ValueError("Potential_Dist must be built with "
                             "calc_forces=True to drive dynamics")
        self.potential = potential
        self.device = torch.device(potential.model.gpus[0])

    def forces(self, structure):
        E, F, _, _ = self.potential.forward(structure)
        return E.detach().reshape(()), F.detach()


def as_force_source(calculator):
    """The protocol object itself, or the adapter for an engine or a
    Potential_Dist."""
    if callable(getattr(calculator, "forces", None)):
        return calculator
    from distmlip_amd.pes import Potential_Dist
    if isinstance(calculator, Potential_Dist):
        return PotentialForces(calculator)
    if callable(getattr(calculator, "step", None)) \
            and hasattr(calculator, "device"):
        return EngineForces(calculator)
    raise TypeError(
        f"{type(calculator).__name__} is no force source: expected an "
        "engine with step(), a Potential_Dist, or an object with "
        "forces(structure) -> (energy, F)")


def _masses_per_atom(masses, species) -> np.ndarray:
    """Per-atom masses (amu) from a scalar, a per-atom array (length N), a
    table indexed by species, or a {species index: mass} dict.  A 1-D array
    of length N is ALWAYS read as per atom, also where it would be a valid
    species table (N atoms of at most N species); pass a dict to force the
    table reading."""
    N = len(species)
    if masses is None:
        raise ValueError("masses are required: Structure carries species "
                         "indices, not elements")
    if isinstance(masses, dict):
        table = np.full(int(max(masses)) + 1, np.nan)
        for k, v in masses.items():
            table[int(k)] = float(v)
        m = table[np.asarray(species, dtype=np.int64)]
    else:
        arr = np.asarray(masses, dtype=np.float64)
        if arr.ndim == 0:
            m = np.full(N, float(arr))
        elif arr.ndim == 1 and len(arr) == N:
            m = arr.copy()
        elif arr.ndim == 1 and len(arr) > int(np.max(species, initial=-1)):
            m = arr[np.asarray(species, dtype=np.int64)]
        else:
            raise ValueError(
                f"masses of shape {arr.shape} are neither per atom (N = {N}) "
                f"nor a table covering species 0..{int(np.max(species))}")
    if not (np.isfinite(m).all() and (m > 0).all()):
        raise ValueError("masses must be finite and positive for every atom")
    return m


# ---------------------------------------------------------------------------
# state
# ---------------------------------------------------------------------------

class MDState:
    """Integrator state on one device: wrapped fp64 `frac` [N,3], cartesian
    `vel` [N,3] (A/fs), `inv_mass` [N] (1/amu; None = unit masses), plus the
    host-side lattice, species and pbc.  72 B per atom (56 with unit masses),
    replicated on every rank."""

    def __init__(self, structure, masses=None, device="cpu",
                 unit_masses: bool = False):
        self.device = torch.device(device)
        self.lattice = np.array(structure.lattice, dtype=np.float64)
        self.linv = np.linalg.inv(self.lattice)
        self.species = np.array(structure.species, dtype=np.int64)
        self.pbc = np.array([1 if int(x) else 0 for x in structure.pbc],
                            dtype=np.int64)
        frac = np.array(structure.frac_coords, dtype=np.float64).reshape(-1, 3)
        for k in range(3):
            if self.pbc[k]:
                f = frac[:, k] - np.floor(frac[:, k])
                frac[:, k] = np.where(f >= 1.0, 0.0, f)
        self.frac = torch.from_numpy(frac).to(self.device)
        self.vel = torch.zeros_like(self.frac)
        if unit_masses:
            self.inv_mass = None
        else:
            m = _masses_per_atom(masses, self.species)
            self.inv_mass = torch.from_numpy(1.0 / m).to(self.device)

    @property
    def num_atoms(self) -> int:
        return self.frac.shape[0]

    def structure(self) -> Structure:
        """Host Structure of the current positions (one D2H copy)."""
        return Structure(frac_coords=self.frac.cpu().numpy(),
                         lattice=self.lattice.copy(),
                         species=self.species.copy(), pbc=self.pbc.copy())

    def kinetic_energy(self) -> float:
        """eV; synchronises."""
        red = md_ops.kick_reduce(self.vel, torch.zeros(
            (self.num_atoms, 3), dtype=torch.float32, device=self.device),
            self.inv_mass, 0.0)
        return 0.5 * float(red[0]) / ACC

    def temperature(self) -> float:
        """K, T = 2 KE / (3 N kB): no degrees of freedom subtracted."""
        return temperature_of(self.kinetic_energy(), self.num_atoms)

    def set_maxwell_boltzmann(self, temperature: float, seed: int = 0):
        """Draw velocities at `temperature` (host generator: the same draw
        on every rank and device), remove the centre-of-mass momentum and
        rescale to exactly `temperature`."""
        if self.inv_mass is None:
            raise ValueError("unit-mass state has no thermal velocities")
        N = self.num_atoms
        gen = torch.Generator(device="cpu")
        gen.manual_seed(int(seed))
        xi = torch.randn((N, 3), dtype=torch.float64, generator=gen)
        im = self.inv_mass.cpu()
        v = xi * torch.sqrt(im * (KB * float(temperature) * ACC)).unsqueeze(1)
        m = 1.0 / im
        v = v - (m.unsqueeze(1) * v).sum(0) / m.sum()
        ke = 0.5 * float((m.unsqueeze(1) * v * v).sum()) / ACC
        if temperature > 0 and ke > 0:
            v = v * math.sqrt(1.5 * N * KB * float(temperature) / ke)
        else:
            v = torch.zeros_like(v)
        self.vel = v.contiguous().to(self.device)


def temperature_of(kinetic: float, n_atoms: int) -> float:
    return 2.0 * kinetic / (3.0 * n_atoms * KB) if n_atoms else 0.0


class Trajectory:
    """Recorded frames: wrapped frac, potential / kinetic / total energy
    (eV) and temperature (K); `save` writes an .npz."""

    def __init__(self):
        self.steps, self.frac = [], []
        self.potential, self.kinetic, self.total, self.temperature = \
            [], [], [], []

    def record(self, step, frac, epot, ekin, temp):
        self.steps.append(int(step))
        self.frac.append(np.array(frac, dtype=np.float64))
        self.potential.append(float(epot))
        self.kinetic.append(float(ekin))
        self.total.append(float(epot) + float(ekin))
        self.temperature.append(float(temp))

    def __len__(self):
        return len(self.steps)

    def as_arrays(self):
        N = self.frac[0].shape[0] if self.frac else 0
        return {"step": np.array(self.steps, dtype=np.int64),
                "frac": (np.stack(self.frac) if self.frac
                         else np.zeros((0, N, 3))),
                "potential": np.array(self.potential),
                "kinetic": np.array(self.kinetic),
                "total": np.array(self.total),
                "temperature": np.array(self.temperature)}

    def save(self, path, **extra):
        with open(path, "wb") as fh:     # np.savez would append ".npz"
            np.savez(fh, **self.as_arrays(), **extra)


# ---------------------------------------------------------------------------
# molecular dynamics
# ---------------------------------------------------------------------------

class MolecularDynamics:
    """MD driver; argument names follow the reference's
    (implementations/matgl/ase.py:228-490).

    ensemble      "nve"           velocity Verlet
                  "nvt"           Berendsen (the reference's default):
                                  lambda = sqrt(1 + dt/taut (T0/T - 1))
                                  (no clipping), applied at the start of a
                                  step from the previous step's kinetic
                                  energy; taut defaults to 100 * timestep
                  "nvt_langevin"  BAOAB, `friction` in 1/fs,
                                  c1 = exp(-friction dt),
                                  c2 = sqrt(kB T ACC (1 - c1^2)); the noise
                                  is torch.randn in fp64 from a generator
                                  seeded with `seed` on the state's device
    masses        amu: a scalar, one per atom (a 1-D array of length N is
                  always read this way), a table indexed by
                  structure.species, or a {species: mass} dict
    timestep      fs;  temperature in K;  taut in fs
    logfile       path or file object; one line every `loginterval` steps
    trajectory    path of an .npz written at the end of every run(), frames
                  every `loginterval` steps (also kept in `.traj`)

    Initial velocities are zero; call
    `md.state.set_maxwell_boltzmann(T, seed)` to thermalise.
    """

    def __init__(self, structure, calculator, masses, ensemble: str = "nvt",
                 temperature: float = 300, timestep: float = 1.0,
                 taut: Optional[float] = None, friction: float = 0.01,
                 seed: int = 0, logfile=None, loginterval: int = 1,
                 trajectory=None):
        ens = str(ensemble).lower()
        if ens not in ENSEMBLES:
            raise ValueError(
                f"unsupported ensemble {ensemble!r}: supported are "
                + ", ".join(repr(e) for e in ENSEMBLES)
                + " (fixed cell only; NPT and the other thermostats of the "
                  "ASE-backed driver are not implemented natively)")
        self.ensemble = ens
        self.source = as_force_source(calculator)
        device = getattr(self.source, "device", "cpu")
        self.state = MDState(structure, masses, device=device)
        self.temperature = float(temperature)
        self.dt = float(timestep)
        if not self.dt > 0:
            raise ValueError("timestep must be positive")
        self.taut = float(taut) if taut is not None else 100.0 * self.dt
        self.friction = float(friction)
        self.loginterval = max(1, int(loginterval))
        self.nsteps = 0
        self.traj = Trajectory()
        self._traj_path = trajectory
        self._own_log = isinstance(logfile, (str, bytes))
        self._log = open(logfile, "a") if self._own_log else logfile
        self._gen = None
        if ens == "nvt_langevin":
            self._gen = torch.Generator(device=self.state.device)
            self._gen.manual_seed(int(seed))
            self._c1 = math.exp(-self.friction * self.dt)
            self._c2 = math.sqrt(KB * self.temperature * ACC
                                 * (1.0 - self._c1 * self._c1))
        self._force = None          # F of the current positions
        self._epot = None           # device scalar or float
        self._kinetic = None        # float, eV, of the current velocities

    # -- scalars (each synchronises) ----------------------------------------

    def _read_kinetic(self, red, step) -> float:
        ke = 0.5 * float(red[0]) / ACC
        if not math.isfinite(ke):
            raise FloatingPointError(
                f"non-finite kinetic energy at MD step {step}")
        return ke

    def _ensure_forces(self):
        if self._force is None:
            self._epot, self._force = self.source.forces(
                self.state.structure())
            red = md_ops.kick_reduce(self.state.vel, self._force,
                                     self.state.inv_mass, 0.0)
            self._kinetic = self._read_kinetic(red, self.nsteps)
            self._record()

    def _record(self):
        epot = float(self._epot)
        temp = temperature_of(self._kinetic, self.state.num_atoms)
        self.traj.record(self.nsteps, self.state.frac.cpu().numpy(), epot,
                         self._kinetic, temp)
        if self._log is not None:
            if len(self.traj) == 1:
                self._log.write("# step time[fs] Etot[eV] Epot[eV] Ekin[eV] "
                                "T[K]\n")
            self._log.write(
                f"{self.nsteps:8d} {self.nsteps * self.dt:12.4f} "
                f"{epot + self._kinetic:18.10f} {epot:18.10f} "
                f"{self._kinetic:16.10f} {temp:12.4f}\n")
            self._log.flush()

    # -- public ---------------------------------------------------------------

    @property
    def potential_energy(self) -> float:
        self._ensure_forces()
        return float(self._epot)

    @property
    def kinetic_energy(self) -> float:
        if self._kinetic is None:
            self._kinetic = self.state.kinetic_energy()
        return self._kinetic

    @property
    def total_energy(self) -> float:
        return self.potential_energy + self.kinetic_energy

    def invalidate(self):
        """Call after changing `state.vel` or `state.frac` by hand."""
        self._force = None
        self._kinetic = None

    def step(self):
        st = self.state
        self._ensure_forces()
        dt = self.dt
        half = 0.5 * dt * ACC
        a = 1.0
        xi, c1, c2 = None, 0.0, 0.0
        if self.ensemble == "nvt":
            # _kinetic is current here: every nvt step reads it, and
            # _ensure_forces() reads it before the first
            T = temperature_of(self._kinetic, st.num_atoms)
            if T > 0.0:
                lam2 = 1.0 + dt / self.taut * (self.temperature / T - 1.0)
                a = math.sqrt(max(lam2, 0.0))
        elif self.ensemble == "nvt_langevin":
            xi = torch.randn((st.num_atoms, 3), dtype=torch.float64,
                             generator=self._gen, device=st.device)
            c1, c2 = self._c1, self._c2
        md_ops.kick_drift(st.frac, st.vel, self._force, st.inv_mass, a, half,
                          dt, st.linv, st.pbc, xi=xi, c1=c1, c2=c2)
        self._epot, self._force = self.source.forces(st.structure())
        red = md_ops.kick_reduce(st.vel, self._force, st.inv_mass, half)
        self.nsteps += 1
        logs = self.nsteps % self.loginterval == 0
        if logs or self.ensemble == "nvt":
            self._kinetic = self._read_kinetic(red, self.nsteps)
        else:
            self._kinetic = None
        if logs:
            self._record()

    def run(self, steps: int):
        for _ in range(int(steps)):
            self.step()
        if self._traj_path is not None:
            self.traj.save(self._traj_path, lattice=self.state.lattice,
                           species=self.state.species, pbc=self.state.pbc)
        return self.traj

    def close(self):
        if self._own_log and self._log is not None:
            self._log.close()
            self._log = None


# ---------------------------------------------------------------------------
# relaxation
# ---------------------------------------------------------------------------

class Relaxer:
    """FIRE at fixed cell with ASE's parameters (dt 0.1, dtmax 1.0, maxstep
    0.2, N_min 5, f_inc 1.1, f_dec 0.5, alpha_start 0.1, f_alpha 0.99, unit
    masses; FIRE's own units, so `masses` is accepted for symmetry with
    MolecularDynamics and not used).

    Per iteration: one kick_reduce(b = 0) gives F.v, |F|^2, |v|^2 and
    max|F_i|^2; the host picks v' = beta v + gamma F (beta = 1 - alpha,
    gamma = alpha |v|/|F| + dt when F.v > 0; beta = 0, gamma = dt otherwise);
    |v'|^2 = beta^2 |v|^2 + 2 beta gamma F.v + gamma^2 |F|^2 gives the
    maxstep clamp s = min(1, maxstep / (dt |v'|)) without a second reduction;
    one kick_drift(a = beta, b = gamma, h = s dt) applies it.  Converged when
    max_i |F_i| < fmax."""

    dt_start, dtmax, maxstep = 0.1, 1.0, 0.2
    n_min, f_inc, f_dec, alpha_start, f_alpha = 5, 1.1, 0.5, 0.1, 0.99

    def __init__(self, calculator, masses=None):
        self.source = as_force_source(calculator)
        self.masses = masses

    def relax(self, structure, fmax: float = 0.1, steps: int = 500,
              traj_file=None, interval: int = 1, relax_cell: bool = False):
        if relax_cell:
            raise NotImplementedError(
                "relax_cell=True: cell relaxation is out of scope of the "
                "native Relaxer (fixed cell only)")
        st = MDState(structure, device=getattr(self.source, "device", "cpu"),
                     unit_masses=True)
        traj = Trajectory()
        interval = max(1, int(interval))
        dt, alpha, n_pos = self.dt_start, self.alpha_start, 0
        converged = False
        it = 0
        while True:
            s_host = st.structure()
            epot, F = self.source.forces(s_host)
            red = md_ops.kick_reduce(st.vel, F, None, 0.0).tolist()
            _, fv, f2, v2, f2max = red
            if not all(math.isfinite(x) for x in red):
                raise FloatingPointError(
                    f"non-finite forces or velocities at FIRE iteration {it}")
            if it % interval == 0:
                traj.record(it, s_host.frac_coords, float(epot), 0.5 * v2, 0.0)
            if math.sqrt(f2max) < fmax:
                converged = True
                break
            if it >= steps:
                break
            if v2 == 0.0:
                # first move (ASE: v is None): v = dt F, nothing adapts
                beta, gamma = 0.0, dt
            elif fv > 0.0:
                # ASE's order: mix with the current alpha, then grow dt and
                # shrink alpha, then kick with the new dt
                beta = 1.0 - alpha
                mix = alpha * math.sqrt(v2 / f2)
                if n_pos > self.n_min:
                    dt = min(dt * self.f_inc, self.dtmax)
                    alpha *= self.f_alpha
                n_pos += 1
                gamma = mix + dt
            else:
                beta = 0.0
                alpha = self.alpha_start
                dt *= self.f_dec
                n_pos = 0
                gamma = dt
            vn2 = beta * beta * v2 + 2.0 * beta * gamma * fv \
                + gamma * gamma * f2
            norm = dt * math.sqrt(max(vn2, 0.0))
            s = self.maxstep / norm if norm > self.maxstep else 1.0
            md_ops.kick_drift(st.frac, st.vel, F, None, beta, gamma, s * dt,
                              st.linv, st.pbc)
            it += 1
        if len(traj) == 0 or traj.steps[-1] != it:
            traj.record(it, s_host.frac_coords, float(epot), 0.5 * v2, 0.0)
        if traj_file is not None:
            traj.save(traj_file, lattice=st.lattice, species=st.species,
                      pbc=st.pbc)
        return {"final_structure": s_host, "trajectory": traj,
                "converged": converged, "nsteps": it,
                "energy": float(epot), "fmax": math.sqrt(f2max)}
