"""GPU tests of the self-recomputing atom-conv block (conv._AtomBlockFn), the
default of checkpointed steps: outputs and gradients against the op-by-op
block under torch.utils.checkpoint (what it replaces) and against fp64
plain torch, with and without the verlet edge mask, as the last block (no
gradient on e2) and as an inner one, two blocks chained, and through
SpmdEngine(checkpoint="on") with the DM_NO_ATOM_BLOCK=1 switch.

The accuracy bound everywhere: max |err| against fp64 at most 2x that of the
op-by-op path on the same inputs, the bound of tests/test_gpu_mlp_tail_bwd.py."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_mlp_tail_bwd import (D, E_SMALL, N_NODES,  # noqa: E402
                                   _bound, _graphs, _mlp)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs HIP GPU")

N_RBF = 9


@pytest.fixture(scope="module")
def graphs():
    return _graphs(torch.device("cuda:0"))


class _Case:
    """Inputs and frozen weights of two chained blocks, fp32 on the GPU."""

    def __init__(self, dev):
        gen = torch.Generator(device="cpu").manual_seed(404)

        def rnd(*shape):
            return torch.randn(*shape, generator=gen).to(dev)

        self.v, self.e = rnd(N_NODES, D), rnd(E_SMALL, D)
        self.bexp = rnd(E_SMALL, N_RBF)
        self.Wbb, self.Wab = rnd(D, N_RBF) / 3, rnd(D, N_RBF) / 3
        self.mask = (torch.rand(E_SMALL, 1, generator=gen) < 0.8).float().to(
            dev)
        self.go_v, self.go_e = rnd(N_NODES, D), rnd(E_SMALL, D)
        self.mlps = [(_mlp(3, dev, 41 + 2 * i), _mlp(3, dev, 42 + 2 * i))
                     for i in range(2)]


@pytest.fixture(scope="module")
def case(graphs):
    return _Case(graphs[0].src.device)


def _run(case, pd, ops, dtype, mode, n_blocks, masked, with_go_e2):
    """(v2, e2, dv, de, dbexp) of n_blocks chained blocks.  mode: "block"
    (_AtomBlockFn), "ckpt" (the op-by-op body under a non-reentrant
    checkpoint, as runtime.atom_conv_body runs), "plain" (the body alone)."""
    from distmlip_amd.chgnet import _packed_weights, gated_mlp_split3
    from distmlip_amd.conv import _AtomBlockFn
    c = case
    v, e, bexp = (t.detach().to(dtype).clone().requires_grad_(True)
                  for t in (c.v, c.e, c.bexp))
    Wbb, Wab = c.Wbb.to(dtype), c.Wab.to(dtype)
    mask = c.mask.to(dtype) if masked else None
    x_v, x_e = v, e
    for m_e, m_n in c.mlps[:n_blocks]:
        m_e, m_n = (copy.deepcopy(m).to(dtype) for m in (m_e, m_n))

        def body(v_, e_, bexp_, m_e=m_e, m_n=m_n):
            wbb, wab = bexp_ @ Wbb.t(), bexp_ @ Wab.t()
            if mask is not None:
                wbb, wab = wbb * mask, wab * mask
            e2 = gated_mlp_split3(m_e, v_, e_, pd, ops, D, w=wbb, base=e_)
            msg = gated_mlp_split3(m_n, v_, e2, pd, ops, D, w=wab)
            return ops.scatter_edges(msg, pd, base=v_), e2

        if mode == "block":
            x_v, x_e = _AtomBlockFn.apply(
                x_v, x_e, bexp, Wbb, Wab, mask, pd, ops,
                _packed_weights(m_e), _packed_weights(m_n), D)
        elif mode == "ckpt":
            x_v, x_e = torch.utils.checkpoint.checkpoint(
                body, x_v, x_e, bexp, use_reentrant=False)
        else:
            x_v, x_e = body(x_v, x_e, bexp)
    loss = (x_v * c.go_v.to(dtype)).sum()
    if with_go_e2:
        loss = loss + (x_e * c.go_e.to(dtype)).sum()
    loss.backward()
    return x_v.detach(), x_e.detach(), v.grad, e.grad, bexp.grad


NAMES = ("v2", "e2", "dv", "de", "dbexp")


@requires_gpu
@pytest.mark.parametrize("n_blocks", [1, 2])
@pytest.mark.parametrize("with_go_e2", [True, False])
@pytest.mark.parametrize("masked", [False, True])
def test_block_vs_checkpoint_and_fp64(monkeypatch, graphs, case, masked,
                                      with_go_e2, n_blocks):
    from distmlip_amd.ops import HipOps
    from oracle.chgnet_ref import CpuRefOps
    pd, pr = graphs
    for name in ("DM_NO_FUSED_MLP1_BWD", "DM_NO_FUSED_MLP_BWD",
                 "DM_NO_FUSED_MLP_FWD", "DM_NO_FUSED_MLP"):
        monkeypatch.delenv(name, raising=False)
    calls = {"bwd": 0, "idx": 0}
    real_bwd, real_tail = HipOps.r_edge_mlp_bwd, HipOps.r_mlp_tail_bwd

    def bwd(self, *a, **k):
        calls["bwd"] += 1
        return real_bwd(self, *a, **k)

    def tail(self, go, cg, w, z, w2, go_idx=None):
        calls["idx"] += go_idx is not None
        return real_tail(self, go, cg, w, z, w2, go_idx)

    # the block's outer forward: both first layers of a block without z
    z_sizes = []
    real_zh = HipOps.edge_mlp3_zh

    def zh(self, *a):
        z, h = real_zh(self, *a)
        z_sizes.append(z.numel())
        return z, h

    monkeypatch.setattr(HipOps, "r_edge_mlp_bwd", bwd)
    monkeypatch.setattr(HipOps, "r_mlp_tail_bwd", tail)
    monkeypatch.setattr(HipOps, "edge_mlp3_zh", zh)
    got = _run(case, pd, HipOps(), torch.float32, "block", n_blocks, masked,
               with_go_e2)
    # two first-layer reverse launches and one indexed tail per block
    assert calls == {"bwd": 2 * n_blocks, "idx": n_blocks}, calls
    assert z_sizes == [0] * (2 * n_blocks), \
        f"outer forward stored z: {z_sizes}"
    # what the block replaces, without the kernels under test: the op-by-op
    # body under a checkpoint with rocBLAS for de
    monkeypatch.setenv("DM_NO_FUSED_MLP1_BWD", "1")
    old = _run(case, pd, HipOps(), torch.float32, "ckpt", n_blocks, masked,
               with_go_e2)
    monkeypatch.delenv("DM_NO_FUSED_MLP1_BWD")
    assert calls == {"bwd": 2 * n_blocks, "idx": n_blocks}, calls
    # (that path records in its outer forward, so it stores z there)
    assert any(z_sizes[2 * n_blocks:]), z_sizes
    ref = _run(case, pr, CpuRefOps(), torch.float64, "plain", n_blocks,
               masked, with_go_e2)
    for name, g, o, r in zip(NAMES, got, old, ref):
        _bound(g, r, o, f"{name} blocks={n_blocks} mask={masked} "
                        f"go_e2={with_go_e2}")


@requires_gpu
def test_block_switch_restores_rocblas(monkeypatch, graphs, case):
    """DM_NO_FUSED_MLP1_BWD=1 inside the block: addmm and r_gather_dst, no
    launch of either new kernel, same bound."""
    import distmlip_amd.ops as ops_mod
    from distmlip_amd.ops import HipOps
    from oracle.chgnet_ref import CpuRefOps
    pd, pr = graphs
    launches = []
    real = ops_mod.raw_edge_mlp_bwd
    monkeypatch.setattr(ops_mod, "raw_edge_mlp_bwd",
                        lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    monkeypatch.setenv("DM_NO_FUSED_MLP1_BWD", "1")
    got = _run(case, pd, HipOps(), torch.float32, "block", 2, False, True)
    old = _run(case, pd, HipOps(), torch.float32, "ckpt", 2, False, True)
    assert not launches
    ref = _run(case, pr, CpuRefOps(), torch.float64, "plain", 2, False, True)
    for name, g, o, r in zip(NAMES, got, old, ref):
        _bound(g, r, o, f"{name} DM_NO_FUSED_MLP1_BWD=1")


# --------------------------------------------------------------------------
# engine level
# --------------------------------------------------------------------------
@requires_gpu
def test_engine_checkpointed(monkeypatch):
    """SpmdEngine(checkpoint="on") on 320 atoms: the default takes the block
    for every atom conv, DM_NO_ATOM_BLOCK=1 takes it for none, and energy
    and forces hold the bound against the fp64 oracle."""
    from distmlip_amd import conv
    from distmlip_amd.model import CHGNetCore
    from distmlip_amd.runtime import SpmdEngine
    from distmlip_amd.structures import diamond_si
    from oracle.chgnet_ref import oracle_forward
    from oracle.graph_ref import brute_force_neighbors
    s = diamond_si((10, 2, 2), jitter=0.1, seed=3)
    core = CHGNetCore.seeded(seed=0).float()
    core64 = copy.deepcopy(core).double()
    n_convs = len(core.atom_convs)
    g = brute_force_neighbors(s.frac_coords, s.lattice, s.pbc, 6.0, 3.0)
    ref = oracle_forward(core64, s, g["src"], g["dst"], g["offsets"],
                         g["within_bond_r"], dtype=torch.float64)
    applies = []
    real = conv._AtomBlockFn.forward
    monkeypatch.setattr(
        conv._AtomBlockFn, "forward",
        staticmethod(lambda *a: (applies.append(1), real(*a))[1]))

    def run():
        eng = SpmdEngine(core, world=1, threads=2, device="cuda:0",
                         checkpoint="on")
        out = eng.step(s)
        F = np.zeros((s.num_atoms, 3))
        F[out["global_ids_owned"]] = \
            out["forces_owned"].double().cpu().numpy()
        return torch.tensor([out["energy"].item()], dtype=torch.float64), \
            torch.from_numpy(F)

    monkeypatch.delenv("DM_NO_ATOM_BLOCK", raising=False)
    E_new, F_new = run()
    assert len(applies) == n_convs, \
        f"{len(applies)} block applies for {n_convs} atom convs"
    monkeypatch.setenv("DM_NO_ATOM_BLOCK", "1")
    E_old, F_old = run()
    assert len(applies) == n_convs, \
        "DM_NO_ATOM_BLOCK=1 still took the block path"
    E64 = torch.tensor([ref["energy"].item()], dtype=torch.float64)
    _bound(F_new, ref["forces"].double(), F_old, "engine forces")
    _bound(E_new, E64, E_old, "engine energy")
