"""TensorNet path correctness on CPU, all fp64.

Parity standard (same as CHGNet and MACE — SURVEY §8(c)): matgl is not
installable and the reference ships no numeric tests, so the dense oracle
(tests/tensornet_ref.py, written from the model definition on
[N, C, 3, 3] tensors) is the executable definition; the product drivers
(TensorNet_Dist, TensorNetSpmdEngine over the component-major
tensornet_ops) must reproduce it, and physics invariants pin the oracle
itself against first principles a restatement cannot fake.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tensornet_ref import message_dense, tensornet_oracle_forward  # noqa: E402

from distmlip_amd.structures import Structure, diamond_si, random_cell  # noqa: E402
from distmlip_amd.tensornet_model import (TensorNetConfig, TensorNetCore,  # noqa: E402
                                          kmajor_rows)
from oracle.chgnet_ref import CpuRefOps  # noqa: E402
from oracle.graph_ref import brute_force_neighbors  # noqa: E402

CUTOFF = 5.0


def _small_core(n_elements=3, seed=0, units=16, group="O(3)"):
    cfg = TensorNetConfig(n_elements=n_elements, units=units, num_rbf=8,
                          cutoff=CUTOFF, group=group, data_mean=0.1,
                          data_std=0.7)
    return TensorNetCore.seeded(cfg, seed=seed).double()


def _graph(s):
    g = brute_force_neighbors(s.frac_coords, s.lattice, s.pbc, CUTOFF, 0.0)
    return g["src"], g["dst"], g["offsets"]


def _si(reps, seed, jitter=0.1):
    s = diamond_si(reps, jitter=jitter, seed=seed)
    s.species = np.arange(s.num_atoms) % 3
    return s


# -- 1. the oracle obeys physics it cannot fake -------------------------------

def test_config_defaults():
    cfg = TensorNetConfig(n_elements=3)
    assert (cfg.units, cfg.nblocks, cfg.num_rbf, cfg.cutoff, cfg.group) == \
        (64, 2, 32, 5.0, "O(3)")
    assert cfg.rbf_width == pytest.approx(31 / 5.0)
    with pytest.raises(TypeError):
        TensorNetConfig()


def test_oracle_translation_invariance():
    s = random_cell(40, a=11.0, n_species=3, seed=1)
    core = _small_core()
    r0 = tensornet_oracle_forward(core, s, *_graph(s))
    s.frac_coords = np.mod(s.frac_coords + np.array([0.13, 0.22, 0.31]), 1.0)
    r1 = tensornet_oracle_forward(core, s, *_graph(s))
    assert abs(r0["energy"].item() - r1["energy"].item()) < 1e-9


@pytest.mark.parametrize("improper", [False, True])
def test_oracle_rotation_invariance_and_force_covariance(improper):
    from distmlip_amd.so3 import random_rotation
    s = random_cell(40, a=11.0, n_species=3, seed=2)
    core = _small_core(seed=3)
    src, dst, off = _graph(s)
    r0 = tensornet_oracle_forward(core, s, src, dst, off)
    R = random_rotation(4)
    if improper:
        R = -R
    assert np.linalg.det(R) == pytest.approx(-1.0 if improper else 1.0)
    s2 = Structure(frac_coords=s.frac_coords.copy(), lattice=s.lattice @ R.T,
                   species=s.species.copy(), pbc=s.pbc.copy())
    r1 = tensornet_oracle_forward(core, s2, src, dst, off)
    assert abs(r0["energy"].item() - r1["energy"].item()) < 1e-9
    dF = np.abs(r1["forces"].numpy() - r0["forces"].numpy() @ R.T).max()
    assert dF < 1e-9, dF


def test_oracle_newton_third_law():
    s = random_cell(40, a=11.0, n_species=3, seed=5)
    r = tensornet_oracle_forward(_small_core(seed=6), s, *_graph(s))
    assert np.abs(r["forces"].numpy().sum(0)).max() < 1e-10


def test_oracle_forces_vs_finite_difference():
    s = random_cell(24, a=10.0, n_species=2, seed=7)
    core = _small_core(n_elements=2, seed=8, units=8)
    src, dst, off = _graph(s)
    r = tensornet_oracle_forward(core, s, src, dst, off)
    inv_lat = np.linalg.inv(s.lattice)
    h = 1e-5
    rng = np.random.default_rng(0)
    base = s.frac_coords.copy()
    for atom in rng.choice(s.num_atoms, 3, replace=False):
        for ax in range(3):
            dm = np.zeros(3)
            dm[ax] = h
            e = []
            for sign in (1.0, -1.0):
                fc = base.copy()
                fc[atom] += sign * dm @ inv_lat
                s.frac_coords = fc
                e.append(tensornet_oracle_forward(
                    core, s, src, dst, off,
                    compute_forces=False)["energy"].item())
            s.frac_coords = base
            fd = -(e[0] - e[1]) / (2 * h)
            got = r["forces"][atom, ax].item()
            assert abs(fd - got) < 1e-5 * max(1.0, abs(got)), (atom, ax)


# -- 2. engine versus oracle ---------------------------------------------------

@pytest.mark.parametrize("group", ["O(3)", "SO(3)"])
def test_engine_vs_oracle(group):
    from distmlip_amd.tensornet_runtime import TensorNetSpmdEngine
    s = _si((6, 2, 2), seed=2)
    core = _small_core(seed=9, group=group)
    eng = TensorNetSpmdEngine(core, world=1, threads=2, device="cpu",
                              ops=CpuRefOps())
    out = eng.step(s, calc_stresses=True)
    ref = tensornet_oracle_forward(core, s, *_graph(s), compute_stress=True)
    assert abs(out["energy"].item() - ref["energy"].item()) < 1e-9
    F = np.zeros((s.num_atoms, 3))
    F[out["global_ids_owned"]] = out["forces_owned"].numpy()
    assert np.abs(F - ref["forces"].numpy()).max() < 1e-9
    assert np.abs(out["stress"].numpy() - ref["stress"].numpy()).max() < 1e-9
    assert np.abs(ref["forces"].numpy()).max() > 1e-3   # not a null model


# -- 3. partition invariance through Potential_Dist ----------------------------

@pytest.fixture(scope="module")
def pes_case():
    s = _si((8, 2, 2), seed=4)
    core = _small_core(seed=11)
    ref = tensornet_oracle_forward(core, s, *_graph(s), compute_stress=True)
    return s, core, ref, {}


@pytest.mark.parametrize("P", [1, 2, 3])
def test_partition_invariance_potential_dist(pes_case, P):
    from distmlip_amd.pes import Potential_Dist
    from distmlip_amd.tensornet import TensorNet_Dist
    s, core, ref, seen = pes_case

    def run(P):
        if P not in seen:
            model = TensorNet_Dist.from_existing(core, dtype=torch.float64)
            model.enable_distributed_mode(
                ["cpu"] * P, ops_factory=lambda dev: CpuRefOps())
            pot = Potential_Dist(model, calc_forces=True, calc_stresses=True,
                                 num_threads=2)
            E, F, S, _ = pot.forward(s)
            seen[P] = (E.item(), F.detach().numpy(), S.detach().numpy())
        return seen[P]

    E1, F1, S1 = run(1)
    E, F, S = run(P)
    assert abs(E - E1) < 1e-10
    assert np.abs(F - F1).max() < 1e-10
    assert np.abs(S - S1).max() < 1e-10
    assert abs(E - ref["energy"].item()) < 1e-9
    assert np.abs(F - ref["forces"].numpy()).max() < 1e-9
    assert np.abs(S - ref["stress"].numpy()).max() < 1e-9


def test_surface_refusals():
    from distmlip_amd.tensornet import TensorNet_Dist
    from distmlip_amd.tensornet_ops import tn_node_energy
    core = _small_core()
    model = TensorNet_Dist.from_existing(core)
    assert model.use_bond_graph is False and model.three_body_cutoff == 0.0
    assert model.cutoff == CUTOFF
    with pytest.raises(NotImplementedError):
        model.predict_structure_dist(None)
    model.enable_distributed_mode(["cpu"],
                                  ops_factory=lambda dev: CpuRefOps())
    with pytest.raises(Exception):
        model.enable_distributed_mode(["cpu"])
    cfg = TensorNetConfig(n_elements=2, units=8, num_rbf=4, is_intensive=True)
    with pytest.raises(NotImplementedError):
        tn_node_energy(TensorNetCore.seeded(cfg), torch.zeros(2, 9, 8))


# -- 4. SPMD over gloo ---------------------------------------------------------

def _worker(rank, world, init_file, out_dir):
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    from distmlip_amd.tensornet_runtime import TensorNetSpmdEngine

    dist.init_process_group("gloo", init_method=f"file://{init_file}",
                            rank=rank, world_size=world)
    try:
        s = _si((12, 2, 2), seed=3, jitter=0.12)
        eng = TensorNetSpmdEngine(_small_core(seed=9), world, threads=2,
                                  device="cpu", ops=CpuRefOps())
        out = eng.step(s, calc_stresses=True)
        np.save(os.path.join(out_dir, f"E_{rank}.npy"),
                np.array([out["energy"].item()]))
        np.save(os.path.join(out_dir, f"F_{rank}.npy"),
                out["forces_owned"].numpy())
        np.save(os.path.join(out_dir, f"gids_{rank}.npy"),
                out["global_ids_owned"])
        np.save(os.path.join(out_dir, f"S_{rank}.npy"),
                out["stress"].numpy())
    finally:
        dist.destroy_process_group()


def test_spmd_gloo_world2_matches_world1(tmp_path):
    from distmlip_amd.tensornet_runtime import TensorNetSpmdEngine
    world = 2
    mp.spawn(_worker, args=(world, str(tmp_path / "pg_init"), str(tmp_path)),
             nprocs=world, join=True)
    s = _si((12, 2, 2), seed=3, jitter=0.12)
    one = TensorNetSpmdEngine(_small_core(seed=9), world=1, threads=2,
                              device="cpu", ops=CpuRefOps()
                              ).step(s, calc_stresses=True)
    F1 = np.zeros((s.num_atoms, 3))
    F1[one["global_ids_owned"]] = one["forces_owned"].numpy()
    F = np.zeros((s.num_atoms, 3))
    covered = np.zeros(s.num_atoms, dtype=bool)
    for r in range(world):
        assert abs(np.load(f"{tmp_path}/E_{r}.npy")[0]
                   - one["energy"].item()) < 1e-9
        gids = np.load(f"{tmp_path}/gids_{r}.npy")
        assert not covered[gids].any()
        covered[gids] = True
        F[gids] = np.load(f"{tmp_path}/F_{r}.npy")
        assert np.abs(np.load(f"{tmp_path}/S_{r}.npy")
                      - one["stress"].numpy()).max() < 1e-9
    assert covered.all()
    assert np.abs(F - F1).max() < 1e-9


# -- 5. algebra of the composition ---------------------------------------------

def test_projection_algebra():
    from distmlip_amd.tensornet_ops import dec9, matmul9, tnorm
    g = torch.Generator().manual_seed(0)
    T = torch.randn(7, 9, 5, dtype=torch.float64, generator=g)
    I, A, S = dec9(T)
    assert (I + A + S - T).abs().max() < 1e-14
    for k, part in enumerate((I, A, S)):
        again = dec9(part)
        for j in range(3):
            want = part if j == k else torch.zeros_like(part)
            assert (again[j] - want).abs().max() < 1e-14, (k, j)
    # plane-wise 3x3 product and norm against the dense forms
    U = torch.randn(7, 9, 5, dtype=torch.float64, generator=g)
    d = lambda X: X.permute(0, 2, 1).reshape(7, 5, 3, 3)     # noqa: E731
    assert (d(matmul9(T, U)) - d(T) @ d(U)).abs().max() < 1e-13
    assert (tnorm(T) - (d(T) ** 2).sum((-2, -1))).abs().max() < 1e-13


def test_kmajor_rows_is_the_matgl_permutation():
    C = 4
    rows = kmajor_rows(C)
    W = torch.arange(3 * C, dtype=torch.float64)           # matgl row ids
    out = W[rows].view(3, C)                               # [k, c] here
    assert torch.equal(out.t().reshape(-1), W)             # (c, k) there


def test_tn_message_matches_dense_oracle():
    from distmlip_amd.tensornet_ops import tn_message

    class PD:
        pass
    g = torch.Generator().manual_seed(1)
    N, E, C = 23, 140, 6
    dst = torch.sort(torch.randint(0, N, (E,), generator=g)).values
    src = torch.randint(0, N, (E,), generator=g)
    pd = PD()
    pd.src, pd.dst, pd.n_atoms = src, dst, N
    Y = torch.randn(N, 9, C, dtype=torch.float64, generator=g,
                    requires_grad=True)
    f = torch.randn(E, 3, C, dtype=torch.float64, generator=g,
                    requires_grad=True)
    M = tn_message(Y, f, pd, CpuRefOps())
    Yd = Y.detach().permute(0, 2, 1).reshape(N, C, 3, 3).requires_grad_(True)
    fd = f.detach().permute(0, 2, 1).clone().requires_grad_(True)  # [E,C,3]
    Md = message_dense(Yd, fd, src, dst, N)
    assert (M.permute(0, 2, 1).reshape(N, C, 3, 3) - Md).abs().max() < 1e-13
    G = torch.randn(N, 9, C, dtype=torch.float64, generator=g)
    gy, gf = torch.autograd.grad((M * G).sum(), [Y, f])
    Gd = G.permute(0, 2, 1).reshape(N, C, 3, 3)
    gyd, gfd = torch.autograd.grad((Md * Gd).sum(), [Yd, fd])
    assert (gy.permute(0, 2, 1).reshape(N, C, 3, 3) - gyd).abs().max() < 1e-13
    assert (gf.permute(0, 2, 1) - gfd).abs().max() < 1e-13
