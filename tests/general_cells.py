"""Shared inputs of the general-lattice GPU graph-build tests
(test_gpu_graph_plan.py on the CPU, test_gpu_graph_general.py on the GPU):
skewed, thin and partly periodic cells, each with one cached brute-force
candidate list and the knife-edge guard over it."""
import functools

import numpy as np

from distmlip_amd.structures import Structure, diamond_si, random_cell

CUTOFF, BOND, TOL = 6.0, 3.0, 1e-8
SHEAR = np.eye(3) + np.array([[0, .08, .05], [0, 0, .1], [0, 0, 0]])


def _open_dims(s, pbc, squeeze=True):
    """pbc flags applied; each open frac coordinate mapped to 0.2 + 0.5 f
    (a cluster / slab / wire strictly inside the cell)."""
    frac = s.frac_coords.copy()
    if squeeze:
        for k in range(3):
            if not pbc[k]:
                frac[:, k] = 0.2 + 0.5 * frac[:, k]
    return Structure(np.ascontiguousarray(frac), s.lattice.copy(),
                     s.species.copy(), np.asarray(pbc, dtype=np.int64))


def mixed_nc():
    rng = np.random.default_rng(3)
    lat = np.array([[30., 0, 0], [3, 13, 0], [1, -1.5, 5]])
    return Structure(np.ascontiguousarray(rng.random((300, 3))), lat,
                     np.zeros(300, dtype=np.int64),
                     np.ones(3, dtype=np.int64))


def shear_si(pbc=(1, 1, 1)):
    s = diamond_si((12, 2, 2), jitter=0.12, seed=2)
    return Structure(s.frac_coords.copy(), s.lattice @ SHEAR,
                     s.species.copy(), np.asarray(pbc, dtype=np.int64))


SHAPES = {
    "skew600": lambda: random_cell(600, a=20.0, seed=11, skew=0.1),
    "thin60": lambda: random_cell(60, a=7.0, seed=12, skew=0.08),
    "tiny12": lambda: random_cell(12, a=4.0, seed=13, skew=0.1),
    "mixed_nc": mixed_nc,
    "pbc110": lambda: _open_dims(
        random_cell(400, a=18.0, seed=21, skew=0.1), (1, 1, 0)),
    "pbc100": lambda: _open_dims(
        random_cell(400, a=18.0, seed=21, skew=0.1), (1, 0, 0)),
    "pbc000": lambda: _open_dims(
        random_cell(400, a=18.0, seed=21, skew=0.1), (0, 0, 0)),
    "pbc011": lambda: _open_dims(
        random_cell(400, a=18.0, seed=21, skew=0.1), (0, 1, 1)),
    "slab24": lambda: _open_dims(
        random_cell(400, a=24.0, seed=21, skew=0.1), (1, 1, 0),
        squeeze=False),
    "shear_si": shear_si,
}
# the plan each shape is meant to stress (None: data-derived, not pinned)
EXPECTED_PLAN = {
    "skew600": ((3, 3, 3), (1, 1, 1)),
    "thin60": ((1, 1, 1), None),
    "tiny12": ((1, 1, 1), (2, 2, 2)),
    "mixed_nc": ((4, 2, 1), (1, 1, 2)),
    "shear_si": ((10, 1, 1), None),
}


@functools.lru_cache(maxsize=None)
def structure(name):
    return SHAPES[name]()


@functools.lru_cache(maxsize=None)
def candidates(name):
    """Every pair (any image) with d < CUTOFF + 0.01, by brute force, the
    d^2 > tol filter disabled: (src, dst, offsets int64[M,3], d2)."""
    from oracle.graph_ref import brute_force_neighbors
    s = structure(name)
    # d2 < r^2 + tol and d2 > tol with tol = -1: keeps 0 <= d2 < r^2 - 1
    r = float(np.sqrt((CUTOFF + 0.01) ** 2 + 1.0))
    g = brute_force_neighbors(s.frac_coords, s.lattice, s.pbc, r, 0.0,
                              tol=-1.0)
    off = np.rint(g["offsets"]).astype(np.int64).reshape(-1, 3)
    return g["src"], g["dst"], off, g["dist"] ** 2


def knife_edge_margin(name):
    """Smallest |d^2 - threshold| over all candidate pairs and the three
    thresholds of the edge test.  A condition on the INPUTS: above 1e-9
    the emit / bond verdicts cannot depend on FMA contraction (the
    difference between two fp64 evaluations of d^2 is ~1e-14 here)."""
    d2 = candidates(name)[3]
    thr = np.array([CUTOFF ** 2 + TOL, BOND ** 2 + TOL, TOL])
    return float(np.abs(d2[:, None] - thr[None, :]).min()) if len(d2) \
        else np.inf


def assert_no_knife_edge(name):
    m = knife_edge_margin(name)
    assert m > 1e-9, f"{name}: a pair sits {m:.2e} from a threshold; " \
        "change the seed"


def brute_edges(name):
    """(src, dst, off) of the true edge set, filtered from candidates()."""
    src, dst, off, d2 = candidates(name)
    keep = (d2 < CUTOFF ** 2 + TOL) & (d2 > TOL)
    return src[keep], dst[keep], off[keep]
