"""The fused fp32-MFMA S2 grid activation (csrc/s2act.hip) against the torch
composition of s2_act in fp64, and the UMA engine through it.

Bound of the fp64 comparisons: 8 x the deviation of the fp32 torch composition
from the same fp64 reference (a different fp32 summation order over up to 512
grid points).  Measured on MI355X, error / that deviation, worst case over
the 27 shapes: forward 1.07, reverse 1.71 (with one sequential chain over all
512 points instead of four the forward reached 8.03).
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs a GPU")]
GRIDS = [(1, 32), (3, 32), (16, 32)]    # one tile, an odd count, the default
NODES = [0, 1, "tile+1", "2tile+3"]     # in units of the block's node tile


def _cfg(C, grid):
    from distmlip_amd.uma_model import UMAConfig
    return UMAConfig(n_elements=3, sphere_channels=C, grid_theta=grid[0],
                     grid_phi=grid[1])


@lru_cache(maxsize=None)
def _case(C, grid, nodes):
    """Operands, the fp64 reference (value, gradient), the kernel's result and
    8 x the fp32 torch composition's own deviation from the reference."""
    from distmlip_amd import uma_ops

    T = uma_ops.s2_n_tile(C)
    N = {0: 0, 1: 1, "tile+1": T + 1, "2tile+3": 2 * T + 3}[nodes]
    cfg = _cfg(C, grid)
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1000 * C + 10 * grid[0] + N)
    x = (2 * torch.randn(N, 9, C, generator=gen)).to(dev)
    lw = torch.randn(N, 9, C, generator=gen).to(dev)

    def run(dt, env):
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("DM_UMA_S2", env)
            a = x.to(dt).requires_grad_(True)
            out = uma_ops.s2_act(a, cfg)
            g = torch.autograd.grad((out * lw.to(dt)).sum(), a)[0] if N \
                else out
        return out.detach().double(), g.detach().double()

    got = run(torch.float32, "hip")
    if N == 0:
        return N, None, got, None
    ref = run(torch.float64, "hip")        # fp64 always takes the composition
    f32 = run(torch.float32, "torch")
    tol = [8 * (a - b).abs().max().item() for a, b in zip(f32, ref)]
    return N, ref, got, tol


@pytest.mark.parametrize("nodes", NODES)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("C", [32, 64, 128])
def test_s2_act_forward_vs_fp64(C, grid, nodes):
    N, ref, got, tol = _case(C, grid, nodes)
    assert got[0].shape == (N, 9, C)
    if N == 0:
        return
    err = (got[0] - ref[0]).abs().max().item()
    print(f"C={C} grid={grid} N={N} fwd err {err:.3e} bound {tol[0]:.3e} "
          f"ratio {8 * err / tol[0]:.2f}")
    assert err <= tol[0]


@pytest.mark.parametrize("nodes", NODES[1:])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("C", [32, 64, 128])
def test_s2_act_reverse_vs_fp64(C, grid, nodes):
    N, ref, got, tol = _case(C, grid, nodes)
    err = (got[1] - ref[1]).abs().max().item()
    print(f"C={C} grid={grid} N={N} dx err {err:.3e} bound {tol[1]:.3e} "
          f"ratio {8 * err / tol[1]:.2f}")
    assert err <= tol[1]


def test_s2_act_repeats_bitwise():
    from distmlip_amd import uma_ops
    cfg = _cfg(64, (16, 32))
    x = (2 * torch.randn(301, 9, 64, device="cuda:0")).requires_grad_(True)
    lw = torch.randn_like(x)
    runs = []
    for _ in range(2):
        out = uma_ops.s2_act(x, cfg)
        runs.append((out.detach(), torch.autograd.grad(out, x, lw)[0]))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("ac,re,rf", [(False, 1e-4, 1e-3), (True, 2e-2, 5e-2)])
def test_s2_act_engine(monkeypatch, ac, re, rf):
    """The engine through the kernel against DM_UMA_S2=torch: fp32 within the
    bounds of test_uma_engine_gpu_chunked_matches, bf16 within the bf16-vs-fp32
    drift bounds of test_uma_engine_bf16_autocast_close; and not the same
    bits, so an inactive dispatch fails."""
    from distmlip_amd.structures import diamond_si
    from distmlip_amd.uma_model import UMAConfig, UMACore
    from distmlip_amd.uma_runtime import UmaSpmdEngine

    s = diamond_si((6, 2, 2), jitter=0.2, seed=3)
    s.species = np.asarray(s.species) % 3
    cfg = UMAConfig(n_elements=3, sphere_channels=64, num_layers=2)
    core = UMACore.seeded(cfg, seed=1).float()
    if ac:          # bf16 input takes the kernel only when asked to
        monkeypatch.setenv("DM_UMA_S2", "hip")
    a = UmaSpmdEngine(core, world=1, threads=4, autocast_bf16=ac).step(s)
    monkeypatch.setenv("DM_UMA_S2", "torch")
    b = UmaSpmdEngine(core, world=1, threads=4, autocast_bf16=ac).step(s)
    e0, e1 = a["energy"].item(), b["energy"].item()
    scale = b["forces_owned"].abs().max().item()
    dF = (a["forces_owned"] - b["forces_owned"]).abs().max().item()
    print(f"bf16={ac} dE {abs(e0 - e1):.3e} dF {dF:.3e} scale {scale:.3e}")
    assert abs(e0 - e1) < re * max(1.0, abs(e1)), (e0, e1)
    assert dF < rf * max(1.0, scale), (dF, scale)
    assert not torch.equal(a["forces_owned"], b["forces_owned"])


@pytest.mark.parametrize("dev,dt,C,grid", [
    ("cpu", torch.float32, 64, (16, 32)), ("cuda:0", torch.float64, 64, (16, 32)),
    ("cuda:0", torch.float32, 48, (16, 32)),
    ("cuda:0", torch.float32, 64, (16, 24))])
def test_s2_act_dispatch_scope(monkeypatch, dev, dt, C, grid):
    from distmlip_amd import uma_ops
    cfg = _cfg(C, grid)
    x = torch.randn(5, 9, C, dtype=dt, device=dev)
    assert not uma_ops.s2_kernel_available(x, cfg)
    got = uma_ops.s2_act(x, cfg)
    monkeypatch.setenv("DM_UMA_S2", "torch")
    assert torch.equal(got, uma_ops.s2_act(x, cfg))
