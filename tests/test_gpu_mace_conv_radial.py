"""Fused MACE convolution with the last radial layer inside
(csrc/mace_conv.hip, dm_mace_conv_rad_*) against an fp64 CPU composition,
and the engine on it against the default path."""
import copy
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs a GPU")
pytestmark = pytest.mark.gpu

# in-edges per dst node (dst-sorted).  In-degrees straddle the 16-edge tile:
# 0, 1, 15, 16, 17, 33, then a few small ones.  Sources run over nodes 0..10,
# so node 11 has no out-edge; 2 -> 2 is a self-loop; rows longer than 11
# repeat edges; node 4 sends 24 edges, so the src rows straddle the tile too
_IN = [[(7 * k + n) % 11 for k in range(d)]
       for n, d in enumerate([0, 1, 15, 16, 17, 16, 2, 3, 5, 4, 1, 6])]
_IN[5] += [4] * 17
# 4 x the max-abs error of the default path (tp_w = h @ Wr.T in fp32 torch,
# conv_fused_hip, dh through autograd) against the same fp64 reference on
# these inputs, the largest of the four cases, measured on an MI355X
# (DESIGN.md §9 addendum 5); the margin covers the MFMA's order over the 64
# terms of w and dh against rocBLAS's
_TOL = {"M": 4 * 9.23e-6, "dxs": 4 * 1.71e-5, "dY": 4 * 1.16e-5,
        "dh": 4 * 1.07e-5}


@lru_cache(maxsize=None)
def _graph():
    src = torch.tensor([s for row in _IN for s in row], dtype=torch.int32)
    dst = torch.tensor([n for n, row in enumerate(_IN) for _ in row],
                       dtype=torch.int32)
    row_ptr = torch.tensor(np.cumsum([0] + [len(r) for r in _IN]),
                           dtype=torch.int32)
    perm = torch.argsort(src.long(), stable=True).to(torch.int32)
    srp = torch.zeros(len(_IN) + 1, dtype=torch.int32)
    srp[1:] = torch.cumsum(torch.bincount(src.long(), minlength=len(_IN)), 0)
    return SimpleNamespace(src=src, dst=dst, row_ptr=row_ptr, src_perm=perm,
                           src_row_ptr=srp)


@lru_cache(maxsize=None)
def _case(layer, C):
    """Inputs (fp32, CPU), cotangents, and the fp64 reference's M and
    gradients."""
    from distmlip_amd import mace_ops, so3
    from distmlip_amd.mace_model import MACEConfig, MACECore
    inter = MACECore.seeded(MACEConfig(n_elements=3, channels=C),
                            seed=0).interactions[layer].requires_grad_(False)
    g, gen = _graph(), torch.Generator().manual_seed(10 * layer + C)
    N, E, P = len(_IN), g.src.numel(), len(inter.paths)
    x = {l: torch.randn(N, C, 2 * l + 1, generator=gen)
         for l in range(layer + 1)}
    Y = so3.real_sh(torch.randn(E, 3, generator=gen))
    h = torch.randn(E, 64, generator=gen)
    cot = {l3: torch.randn(N, C, 2 * l3 + 1, generator=gen)
           for l3 in range(4)}
    xr = {l: t.double().requires_grad_(True) for l, t in x.items()}
    Yr, hr = (t.double().requires_grad_(True) for t in (Y, h))
    w = (hr @ inter.radial.layers[-1].weight.double().t()).view(E, P, C)
    msgs = mace_ops.conv_tp_messages(
        inter, {l: t[g.src.long()] for l, t in xr.items()}, Yr, w)
    M = {l3: torch.zeros(N, C, 2 * l3 + 1, dtype=torch.float64).index_add_(
        0, g.dst.long(), m) for l3, m in msgs.items()}
    sum((M[l3] * cot[l3].double()).sum() for l3 in M).backward()
    ref = {"M": M, "dxs": {l: t.grad for l, t in xr.items()},
           "dY": Yr.grad, "dh": hr.grad}
    return inter, x, Y, h, cot, ref


def _run(layer, C, radial=True):
    """M and the leaves with their gradients: the new path, or the default
    one (radial=False) that the tolerances were measured on."""
    from distmlip_amd import mace_ops
    inter, x, Y, h, cot, _ = _case(layer, C)
    dev = torch.device("cuda:0")
    inter = copy.deepcopy(inter).to(dev)
    pd = SimpleNamespace(**{k: v.to(dev) for k, v in vars(_graph()).items()})
    xk = {l: t.to(dev).requires_grad_(True) for l, t in x.items()}
    Yk, hk = (t.to(dev).requires_grad_(True) for t in (Y, h))
    if radial:
        M = mace_ops.conv_radial_hip(inter, xk, Yk, hk, pd)
    else:
        w = (hk @ inter.radial.layers[-1].weight.t()).view(
            -1, len(inter.paths), C)
        M = mace_ops.conv_fused_hip(inter, xk, Yk, w, pd)
    sum((M[l3] * cot[l3].to(dev)).sum() for l3 in M).backward()
    return M, xk, Yk, hk


def _errors(M, xk, Yk, hk, ref):
    """max-abs error of each quantity against the fp64 reference."""
    err = lambda a, b: (a.detach().double().cpu() - b).abs().max().item()
    return {"M": max(err(M[l3], ref["M"][l3]) for l3 in M),
            "dxs": max(err(xk[l].grad, ref["dxs"][l]) for l in xk),
            "dY": err(Yk.grad, ref["dY"]), "dh": err(hk.grad, ref["dh"])}


@requires_gpu
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("layer", [0, 1])
def test_conv_radial_vs_fp64(layer, C):
    M, xk, Yk, hk = _run(layer, C)
    errs = _errors(M, xk, Yk, hk, _case(layer, C)[-1])
    print(layer, C, errs)
    for k, e in errs.items():
        assert e <= _TOL[k], (layer, C, k, e, _TOL[k])
    for l3 in M:                      # node 0 has no in-edge
        assert M[l3][0].abs().max().item() == 0.0, l3
    for l in xk:                      # node 11 has no out-edge
        assert xk[l].grad[11].abs().max().item() == 0.0, l
    M2, xk2, Yk2, hk2 = _run(layer, C)
    assert all(torch.equal(M[l3], M2[l3]) for l3 in M)
    assert all(torch.equal(xk[l].grad, xk2[l].grad) for l in xk)
    assert torch.equal(Yk.grad, Yk2.grad) and torch.equal(hk.grad, hk2.grad)


@requires_gpu
def test_mace_engine_radial_matches_default(monkeypatch):
    from distmlip_amd.mace_model import MACEConfig, MACECore
    from distmlip_amd.mace_runtime import MaceSpmdEngine
    from distmlip_amd.ops import hip_lib
    from distmlip_amd.structures import diamond_si

    s = diamond_si((6, 2, 2), jitter=0.1, seed=3)
    s.species = np.asarray(s.species) % 3
    core = MACECore.seeded(MACEConfig(n_elements=3, channels=64),
                           seed=1).float()
    eng = MaceSpmdEngine(core, world=1, threads=4)
    calls = {"dm_mace_conv_fwd_f32": 0, "dm_mace_conv_rad_fwd_f32": 0}

    def count(name):
        real = getattr(hip_lib(), name)

        def wrapped(*a):
            calls[name] += 1
            return real(*a)
        monkeypatch.setattr(hip_lib(), name, wrapped, raising=False)
    for name in calls:
        count(name)
    default = eng.step(s)
    L = len(core.interactions)
    assert calls == {"dm_mace_conv_fwd_f32": L, "dm_mace_conv_rad_fwd_f32": 0}
    monkeypatch.setenv("DM_MACE_CONV", "radial")
    a, b = eng.step(s), eng.step(s)
    # 192 atoms with some 46 neighbours each: far more than 3000 edges, and
    # still one kernel per interaction
    monkeypatch.setenv("DM_MACE_CHUNK", "3000")
    c = eng.step(s)
    assert calls == {"dm_mace_conv_fwd_f32": L,
                     "dm_mace_conv_rad_fwd_f32": 3 * L}
    e0 = default["energy"].item()
    assert abs(a["energy"].item() - e0) < 1e-4 * max(1.0, abs(e0))
    dF = (a["forces_owned"] - default["forces_owned"]).abs().max().item()
    assert dF < 1e-4, dF
    assert torch.equal(a["forces_owned"], b["forces_owned"])
    assert torch.equal(a["forces_owned"], c["forces_owned"])
