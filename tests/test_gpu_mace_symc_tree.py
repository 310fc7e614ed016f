"""Tree-factored MACE symmetric contraction (csrc/mace_symc.hip) against the
fp64 CPU composition, its dispatch, and the engine on it."""
import copy
from functools import lru_cache

import numpy as np
import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")
pytestmark = pytest.mark.gpu

N = 7            # not a multiple of the waves per block; all 3 elements
# 4 x the max-abs error, against the same fp64 reference on these inputs, of
# the path that served them before this kernel: dm_mace_symc_* at C = 64 and
# 128, the fp32 torch composition on the GPU at C = 192; the largest of the
# six cases, measured on an MI355X (DESIGN.md §9 addendum 6).  The margin
# covers another summation order over at most a few hundred terms.  The new
# kernel's own largest errors there: out 8.66e-7, dx 1.48e-6.
_TOL = {"out": 4 * 1.84e-5, "dx": 4 * 7.95e-6}
# the same rule for the engine: |dE| and max |dF| between DM_MACE_SYMC=torch
# and the flat kernel at C = 128 on the structure below were 0 (the fp32
# energies are equal) and 2.13e-14 (forces there are of order 3e-8); the new
# kernel at C = 192 measured 0 and 1.67e-15
_TOL_E, _TOL_F = 4 * 0.0, 4 * 2.13e-14


@lru_cache(maxsize=None)
def _case(layer, C):
    """Frozen product block, inputs (fp32, CPU), cotangents and the fp64
    reference's out and dx."""
    from distmlip_amd import mace_ops
    from distmlip_amd.mace_model import MACEConfig, MACECore
    core = MACECore.seeded(MACEConfig(n_elements=3, channels=C), seed=0)
    core.requires_grad_(False)
    prod, corr = core.products[layer], core.config.correlation
    gen = torch.Generator().manual_seed(10 * layer + C)
    x = {l: torch.randn(N, C, 2 * l + 1, generator=gen) for l in range(4)}
    species = torch.arange(N) % 3
    cot = {lo: torch.randn(N, C, 2 * lo + 1, generator=gen)
           for lo in prod.out_ls}
    xr = {l: t.double().requires_grad_(True) for l, t in x.items()}
    core.double()
    out = mace_ops.symmetric_contract(prod, xr, species, corr)
    sum((out[lo] * cot[lo].double()).sum() for lo in out).backward()
    ref = {"out": {lo: t.detach() for lo, t in out.items()},
           "dx": {l: t.grad for l, t in xr.items()}}
    core.float()
    return prod, corr, x, species, cot, ref


def _errors(contract, layer, C):
    """max-abs error of out and dx of contract(prod, x, species, corr) on the
    GPU against the fp64 reference."""
    prod, corr, x, species, cot, ref = _case(layer, C)
    dev = torch.device("cuda:0")
    prod = copy.deepcopy(prod).to(dev)
    xk = {l: t.to(dev).requires_grad_(True) for l, t in x.items()}
    out = contract(prod, xk, species.to(dev), corr)
    sum((out[lo] * cot[lo].to(dev)).sum() for lo in out).backward()
    err = lambda a, b: (a.detach().double().cpu() - b).abs().max().item()
    return {"out": max(err(out[lo], ref["out"][lo]) for lo in out),
            "dx": max(err(xk[l].grad, ref["dx"][l]) for l in xk)}


@requires_gpu
@pytest.mark.parametrize("C", [64, 128, 192])
@pytest.mark.parametrize("layer", [0, 1])
def test_symc_tree_vs_fp64(layer, C):
    from distmlip_amd import mace_ops
    errs = _errors(mace_ops.symmetric_contract_tree, layer, C)
    print(layer, C, errs)
    for k, e in errs.items():
        assert e <= _TOL[k], (layer, C, k, e, _TOL[k])


@requires_gpu
def test_symc_tree_dispatch(monkeypatch):
    from distmlip_amd import mace_ops
    from distmlip_amd.ops import hip_lib
    calls = []
    real = hip_lib().dm_mace_symc_tree_fwd_f32
    monkeypatch.setattr(
        hip_lib(), "dm_mace_symc_tree_fwd_f32",
        lambda *a: calls.append(1) or real(*a), raising=False)
    dev = torch.device("cuda:0")

    def run(C, n=N):
        prod, corr, x, species, _, _ = _case(0, C)
        return mace_ops.symmetric_contract(
            copy.deepcopy(prod).to(dev), {l: t[:n].to(dev) for l, t in x.items()},
            species[:n].to(dev), corr)

    monkeypatch.delenv("DM_MACE_SYMC", raising=False)
    a, b = run(192), run(192)
    assert len(calls) == 2
    for lo in a:                      # bit-equal from run to run
        assert torch.equal(a[lo], b[lo]), lo
    empty = run(192, n=0)
    assert {lo: tuple(t.shape) for lo, t in empty.items()} == \
        {0: (0, 192, 1), 1: (0, 192, 3)}
    del calls[:]
    run(128)
    assert not calls
    monkeypatch.setenv("DM_MACE_SYMC", "tree")
    run(128)
    assert len(calls) == 1


@requires_gpu
def test_mace_engine_symc_tree_matches_torch(monkeypatch):
    from distmlip_amd.mace_model import MACEConfig, MACECore
    from distmlip_amd.mace_runtime import MaceSpmdEngine
    from distmlip_amd.ops import hip_lib
    from distmlip_amd.structures import diamond_si

    s = diamond_si((6, 2, 2), jitter=0.1, seed=3)
    s.species = np.asarray(s.species) % 3
    core = MACECore.seeded(MACEConfig(n_elements=3, channels=192),
                           seed=1).float()
    eng = MaceSpmdEngine(core, world=1, threads=4)
    calls = []
    real = hip_lib().dm_mace_symc_tree_fwd_f32
    monkeypatch.setattr(
        hip_lib(), "dm_mace_symc_tree_fwd_f32",
        lambda *a: calls.append(1) or real(*a), raising=False)
    monkeypatch.delenv("DM_MACE_SYMC", raising=False)
    a = eng.step(s)
    assert len(calls) == len(core.products)
    monkeypatch.setenv("DM_MACE_SYMC", "torch")
    ref = eng.step(s)
    assert len(calls) == len(core.products)
    dE = abs(a["energy"].item() - ref["energy"].item())
    dF = (a["forces_owned"] - ref["forces_owned"]).abs().max().item()
    print(dE, dF)
    assert dE <= _TOL_E and dF <= _TOL_F, (dE, dF)
