"""Host side of the general-lattice GPU graph build (no GPU needed):
scope guard, dispatch predicate, and the fractional-space cell plan —
coverage of every brute-force edge by the planned stencil, and a numpy
emulation of the kernel's unwrapped-index enumeration (each (neighbor,
image) pair exactly once, for nc = 1, 2 and >= 3 alike)."""
import numpy as np
import pytest

import general_cells as gc
from distmlip_amd import gpu_graph
from distmlip_amd.structures import Structure, bcc_li, diamond_si, random_cell


def _plan(s):
    return gpu_graph.cell_plan(s.lattice, s.pbc, s.frac_coords, gc.CUTOFF,
                               gc.TOL)


@pytest.mark.parametrize("name", sorted(gc.SHAPES))
def test_supported_on_general_cells(name):
    s = gc.structure(name)
    assert gpu_graph.supported(s, gc.CUTOFF)
    assert not gpu_graph.fast_scope(s.lattice, s.pbc, gc.CUTOFF)
    assert gpu_graph.engages(s, gc.CUTOFF, "auto")
    assert not gpu_graph.engages(s, gc.CUTOFF, "fast")
    assert not gpu_graph.engages(s, gc.CUTOFF, "off")


@pytest.mark.parametrize("name", sorted(gc.EXPECTED_PLAN))
def test_plan_hits_the_stressed_regime(name):
    nc, R, _, _ = _plan(gc.structure(name))
    want_nc, want_R = gc.EXPECTED_PLAN[name]
    assert tuple(nc) == want_nc
    if want_R is not None:
        assert tuple(R) == want_R


def test_open_dims_have_data_derived_extent():
    for name in ("pbc110", "pbc100", "pbc000", "pbc011"):
        s = gc.structure(name)
        nc, R, origin, span = _plan(s)
        for k in range(3):
            if s.pbc[k]:
                assert origin[k] == 0.0 and span[k] == 1.0
            else:
                assert origin[k] == s.frac_coords[:, k].min()
                assert 0.45 < span[k] <= 0.5
                assert nc[k] == 1 and R[k] == 0
    nc, R, _, span = _plan(gc.structure("slab24"))
    assert nc[2] >= 3 and R[2] == 1 and span[2] > 0.9


def test_unsupported_falls_back():
    s = gc.structure("skew600")
    sing = Structure(s.frac_coords, s.lattice.copy(), s.species, s.pbc)
    sing.lattice[2] = sing.lattice[0] + sing.lattice[1]
    assert not gpu_graph.supported(sing, gc.CUTOFF)
    # 0.04 A cell: image index ceil(rc / h) = 151 > 127 leaves int8
    short = Structure(s.frac_coords[:4], np.diag([20.0, 20.0, 0.04]),
                      s.species[:4], s.pbc)
    assert not gpu_graph.supported(short, gc.CUTOFF)
    # ... but the same cell left open in z needs no images at all
    short.pbc = np.array([1, 1, 0])
    assert gpu_graph.supported(short, gc.CUTOFF)
    frac = s.frac_coords.copy()
    frac[7, 1] = 1.2
    unwrapped = Structure(frac, s.lattice, s.species, s.pbc)
    assert not gpu_graph.supported(unwrapped, gc.CUTOFF)
    # an open dim carries no wrap contract
    unwrapped.pbc = np.array([1, 0, 1])
    assert gpu_graph.supported(unwrapped, gc.CUTOFF)
    with pytest.raises(ValueError):
        gpu_graph.engages(s, gc.CUTOFF, "sometimes")


def test_expected_edge_count_guard():
    """N * expected neighbours within a factor 2 of the int32 edge arrays:
    fall back instead of building."""
    rng = np.random.default_rng(0)
    frac = rng.random((200_000, 3))
    dense = Structure(frac, np.diag([30.0, 30.0, 30.0]) + 0.5,
                      np.zeros(len(frac), dtype=np.int64), np.ones(3, int))
    # 2e5 atoms * (2e5 / 27000 A^3) * 905 A^3 = 1.3e9 expected edges
    assert not gpu_graph.supported(dense, gc.CUTOFF)


@pytest.mark.parametrize("name", ["bcc_li8", "si_12_4_4"])
def test_fast_scope_unchanged(name):
    s = bcc_li(8, jitter=0.12, seed=4) if name == "bcc_li8" \
        else diamond_si((12, 4, 4), jitter=0.12, seed=2)
    assert gpu_graph.fast_scope(s.lattice, s.pbc, gc.CUTOFF)
    assert gpu_graph.supported(s, gc.CUTOFF)
    assert gpu_graph.engages(s, gc.CUTOFF, "fast")
    nc, R, origin, span = _plan(s)
    L = np.diag(s.lattice)
    assert tuple(R) == (1, 1, 1)
    assert tuple(nc) == tuple(int(x) for x in np.floor(L / gc.CUTOFF))
    assert (origin == 0).all() and (span == 1).all()
    # one condition away from the old scope -> general kernels
    assert not gpu_graph.fast_scope(s.lattice, [1, 1, 0], gc.CUTOFF)
    sheared = s.lattice.copy()
    sheared[1, 0] = 0.3
    assert not gpu_graph.fast_scope(sheared, s.pbc, gc.CUTOFF)
    thin = diamond_si((12, 2, 2), jitter=0.12, seed=2)
    assert not gpu_graph.fast_scope(thin.lattice, thin.pbc, gc.CUTOFF)
    assert gpu_graph.supported(thin, gc.CUTOFF)


def test_cell_cap_keeps_stencil_valid():
    """A sparse huge box: the cap shrinks nc (bigger cells), R stays."""
    s = random_cell(50, a=4000.0, seed=1, skew=0.05)
    nc0, R0, _, _ = _plan(s)
    assert int(nc0.prod()) > 10 ** 8
    nc, R, _, _ = gpu_graph.cell_plan(s.lattice, s.pbc, s.frac_coords,
                                      gc.CUTOFF, gc.TOL, max_cells=4096)
    assert int(nc.prod()) <= 4096 and (nc >= 1).all() and (nc <= nc0).all()
    assert tuple(R) == tuple(R0) == (1, 1, 1)


@pytest.mark.parametrize("name", sorted(gc.SHAPES))
def test_plan_covers_every_brute_force_edge(name):
    gc.assert_no_knife_edge(name)
    s = gc.structure(name)
    nc, R, origin, span = _plan(s)
    cell = gpu_graph.cell_index(s.frac_coords, nc, origin, span)
    src, dst, off = gc.brute_edges(name)
    assert len(src) > 0
    for k in range(3):
        if s.pbc[k]:
            unwrapped = cell[dst, k] + off[:, k] * nc[k]
        else:
            assert (off[:, k] == 0).all()
            assert cell[:, k].min() >= 0 and cell[:, k].max() < nc[k]
            unwrapped = cell[dst, k]
        assert np.abs(unwrapped - cell[src, k]).max() <= R[k], (name, k)


def _emulate_kernel(s, nc, R, origin, span):
    """numpy restatement of k_nl_gen's enumeration: unwrapped indices,
    floor-div image folding, open-boundary skip.  Returns edge tuples
    (src=j, dst=c, off=-m) in emission order."""
    pbc = [bool(int(x)) for x in s.pbc]
    pos = s.frac_coords @ s.lattice
    cell = gpu_graph.cell_index(s.frac_coords, nc, origin, span)
    cid = (cell[:, 0] * nc[1] + cell[:, 1]) * nc[2] + cell[:, 2]
    members = {}
    for a in np.argsort(cid, kind="stable"):
        members.setdefault(int(cid[a]), []).append(int(a))
    members = {k: np.asarray(v) for k, v in members.items()}
    r2tol = gc.CUTOFF ** 2 + gc.TOL
    out = []
    for c in range(len(pos)):
        for dx in range(-R[0], R[0] + 1):
            for dy in range(-R[1], R[1] + 1):
                for dz in range(-R[2], R[2] + 1):
                    a = cell[c] + np.array([dx, dy, dz])
                    m = np.zeros(3, dtype=np.int64)
                    skip = False
                    for k in range(3):
                        if pbc[k]:
                            m[k] = a[k] // nc[k]
                            a[k] -= m[k] * nc[k]
                        elif a[k] < 0 or a[k] >= nc[k]:
                            skip = True
                    if skip:
                        continue
                    js = members.get(int((a[0] * nc[1] + a[1]) * nc[2]
                                         + a[2]))
                    if js is None:
                        continue
                    js = js[js != c]
                    d = pos[js] + m @ s.lattice - pos[c]
                    d2 = (d * d).sum(1)
                    for j in js[(d2 < r2tol) & (d2 > gc.TOL)]:
                        out.append((int(j), c, -int(m[0]), -int(m[1]),
                                    -int(m[2])))
    return out


@pytest.mark.parametrize("name", ["thin60", "tiny12", "mixed_nc", "pbc100",
                                  "slab24", "shear_si"])
def test_stencil_enumeration_is_exact(name):
    """nc = 1 (thin60, tiny12 with R = 2), nc = 2 (mixed_nc), open dims
    with one cell (pbc100) and several (slab24): the enumeration gives the
    brute-force edge set with no duplicate."""
    gc.assert_no_knife_edge(name)
    s = gc.structure(name)
    got = _emulate_kernel(s, *_plan(s))
    assert len(got) == len(set(got))
    src, dst, off = gc.brute_edges(name)
    # oracle edge (src=i, dst=j, o): bv = pos_j + o L - pos_i; the kernel
    # emits centre as dst with off = -m, i.e. the reversed edge
    want = set(zip(dst.tolist(), src.tolist(), (-off[:, 0]).tolist(),
                   (-off[:, 1]).tolist(), (-off[:, 2]).tolist()))
    assert set(got) == want
