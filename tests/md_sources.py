"""Analytic force sources for the MD driver tests (the `forces(structure)`
protocol of distmlip_amd/md.py), shared by the CPU and GPU test files."""
import math

import numpy as np
import torch

from distmlip_amd import gpu_graph
from distmlip_amd.md import ACC
from distmlip_amd.structures import Structure

TRICLINIC = np.array([[8.0, 0.0, 0.0], [1.0, 7.0, 0.0], [0.5, -0.7, 6.0]])
K_SPRING = 2.0          # eV/A^2
MASS_SI = 28.0855       # amu


class ZeroForces:
    def __init__(self, device="cpu"):
        self.device = torch.device(device)

    def forces(self, structure):
        return 0.0, torch.zeros((structure.num_atoms, 3), dtype=torch.float32,
                                device=self.device)


class EinsteinCrystal:
    """F = -k * (minimal-image displacement from the atom's own site), fp64,
    evaluated on `device`.  E = k/2 sum |d|^2."""

    def __init__(self, site_frac, lattice, k=K_SPRING, device="cpu"):
        self.device = torch.device(device)
        self.k = float(k)
        self.site = torch.as_tensor(np.asarray(site_frac), dtype=torch.float64,
                                    device=self.device)
        self.lat = torch.as_tensor(np.asarray(lattice), dtype=torch.float64,
                                   device=self.device)
        self.calls = 0

    def displacement(self, frac):
        df = torch.as_tensor(np.asarray(frac), dtype=torch.float64,
                             device=self.device) - self.site
        df = df - torch.round(df)
        return df @ self.lat

    def forces(self, structure):
        self.calls += 1
        d = self.displacement(structure.frac_coords)
        return 0.5 * self.k * (d * d).sum(), -self.k * d


def einstein_setup(seed=0, n=64, sigma=0.15, lattice=TRICLINIC):
    """64 random sites, eight of them at frac (0, 0.999, 0.5) so that atoms
    cross cell faces; returns (sites, d0 [n,3] cartesian, start Structure)."""
    rng = np.random.default_rng(seed)
    site = rng.random((n, 3))
    site[:8] = np.array([0.0, 0.999, 0.5])
    d0 = rng.normal(0.0, sigma, (n, 3))
    frac = site + d0 @ np.linalg.inv(lattice)
    frac = frac - np.floor(frac)
    frac[frac >= 1.0] = 0.0
    s = Structure(frac_coords=frac, lattice=np.array(lattice),
                  species=np.zeros(n, dtype=np.int64),
                  pbc=np.ones(3, dtype=np.int64))
    return site, d0, s


def verlet_cos_theta(dt, k=K_SPRING, mass=MASS_SI):
    """Velocity Verlet on a harmonic well from rest: d_n = d_0 cos(n theta)
    with cos(theta) = 1 - w^2 dt^2 / 2, w^2 = k ACC / m."""
    return 1.0 - 0.5 * (k * ACC / mass) * dt * dt


def check_exact_verlet(md, source, d0, dt, nsteps):
    """Step `md` nsteps times; returns (max |d_n - d_0 cos(n theta)| in A,
    number of wrap events)."""
    theta = math.acos(verlet_cos_theta(dt))
    worst, wraps = 0.0, 0
    prev = md.state.frac.cpu().numpy().copy()
    for n in range(1, nsteps + 1):
        md.step()
        frac = md.state.frac.cpu().numpy()
        wraps += int((np.abs(frac - prev) > 0.5).sum())
        prev = frac.copy()
        d = source.displacement(frac).cpu().numpy()
        worst = max(worst, float(np.abs(d - d0 * math.cos(n * theta)).max()))
    return worst, wraps


# -- the periodic wrap ----------------------------------------------------------

WRAP_CASES = [      # (start, displacement in frac) -> wrapped
    (0.0, -1e-17, 0.0),        # x - floor(x) alone would give exactly 1.0
    (0.5, 0.5, 0.0),           # exactly 1.0
    (0.5, 2.25, 0.75),
    (0.75, -4.0, 0.75),        # -3.25
]


def wrap_table(kick_drift, device):
    """One atom per case in a cubic 10 A cell, moved along x by a unit
    'force' kick (a = 0, b = 1, h = 1: dr = F).  Returns (periodic result,
    open-dim result) as numpy [4]."""
    lat = np.eye(3) * 10.0
    linv = np.linalg.inv(lat)
    out = []
    for pbc in ((1, 1, 1), (0, 1, 1)):
        frac = torch.tensor([[c[0], 0.25, 0.5] for c in WRAP_CASES],
                            dtype=torch.float64, device=device)
        vel = torch.zeros_like(frac)
        # dr_x * 0.1 must reproduce the fractional displacement exactly
        F = torch.zeros_like(frac)
        F[:, 0] = torch.tensor([c[1] for c in WRAP_CASES],
                               dtype=torch.float64) / 0.1
        assert (F[:, 0].cpu() * 0.1).tolist() == [c[1] for c in WRAP_CASES]
        kick_drift(frac, vel, F, None, 0.0, 1.0, 1.0, linv, pbc)
        assert frac[:, 1:].cpu().tolist() == [[0.25, 0.5]] * len(WRAP_CASES)
        out.append(frac[:, 0].cpu().numpy())
    return out


def check_wrap_table(periodic, open_):
    for (start, d, want), got, raw in zip(WRAP_CASES, periodic, open_):
        assert got == want, (start, d, got)
        assert 0.0 <= got < 1.0
        assert raw == start + d, (start, d, raw)      # left unwrapped
    assert open_[0] < 0.0 and open_[1] == 1.0
    # the graph builder takes the wrapped coordinates
    frac = np.stack([periodic, np.full(4, 0.25), np.full(4, 0.5)], axis=1)
    s = Structure(frac_coords=frac, lattice=np.eye(3) * 10.0,
                  species=np.zeros(4, dtype=np.int64),
                  pbc=np.ones(3, dtype=np.int64))
    assert gpu_graph.supported(s, 6.0)
