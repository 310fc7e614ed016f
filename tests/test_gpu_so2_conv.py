"""The fused bf16-MFMA SO(2) convolution (csrc/so2.hip) against so2_conv in
fp64 on bf16-representable operands, where the kernel differs from the
reference by fp32 summation order only; and the bf16 engine mode through it."""
import copy
from functools import lru_cache

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs a GPU")]
T = 64                                  # the kernel's edge tile


@lru_cache(maxsize=None)
def _case(C, E):
    """Operands, the fp64 reference (value and gradients) and the fp32 torch
    path's own deviations from it (the yardstick of the bounds)."""
    from distmlip_amd import uma_ops
    from distmlip_amd.uma_model import UMAConfig, UMACore

    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(100 * C + E)
    core = UMACore.seeded(UMAConfig(n_elements=3, sphere_channels=C), seed=0)
    conv = copy.deepcopy(core.blocks[0].msg).requires_grad_(False)
    for p in conv.parameters():
        p.copy_(p.bfloat16().float())
    conv = conv.to(dev)

    def rep(*shape, uniform=False):
        t = torch.rand(*shape, generator=gen) if uniform \
            else torch.randn(*shape, generator=gen)
        return t.bfloat16().float().to(dev)

    xs, xd, lw = rep(E, 9, C), rep(E, 9, C), rep(E, 9, C)
    gate = rep(E, 3, uniform=True)

    def run(fn, dt):
        a = [t.to(dt).requires_grad_(True) for t in (xs, xd, gate)]
        out = fn(*a)
        grads = torch.autograd.grad((out * lw.to(dt)).sum(), a) if E else ()
        return [out.detach().double()] + [g.double() for g in grads]

    got = run(lambda s, d, g: uma_ops.so2_conv_fused(conv, s, d, g),
              torch.float32)
    if E == 0:                 # the torch forms cannot reshape zero rows
        return None, got, None
    conv64 = copy.deepcopy(conv).double()
    ref = run(lambda s, d, g: uma_ops.so2_conv(
        conv64, torch.cat([s, d], 2), g, C), torch.float64)
    f32 = run(lambda s, d, g: uma_ops.so2_conv_split(conv, s, d, g, C),
              torch.float32)
    tol = [8 * (a - b).abs().max().item() for a, b in zip(f32, ref)]
    return ref, got, tol


@pytest.mark.parametrize("E", [0, 1, T + 1, 2 * T + 17])
@pytest.mark.parametrize("C", [64, 128])
def test_so2_fused_forward_vs_fp64(C, E):
    ref, got, tol = _case(C, E)
    assert got[0].shape == (E, 9, C)
    if E == 0:
        return
    err = (got[0] - ref[0]).abs().max().item()
    print(f"C={C} E={E} fwd err {err:.3e} bound {tol[0]:.3e}")
    assert err <= tol[0]


@pytest.mark.parametrize("E", [1, T + 1, 2 * T + 17])
@pytest.mark.parametrize("C", [64, 128])
def test_so2_fused_reverse_vs_fp64(C, E):
    ref, got, tol = _case(C, E)
    errs = [(g - r).abs().max().item() for g, r in zip(got[1:], ref[1:])]
    print(f"C={C} E={E} dxs/dxd/dgate err {errs} bounds {tol[1:]}")
    for name, e, t in zip(("dxs", "dxd", "dgate"), errs, tol[1:]):
        assert e <= t, (name, e, t)


def _engine_step(ac):
    from distmlip_amd.structures import diamond_si
    from distmlip_amd.uma_model import UMAConfig, UMACore
    from distmlip_amd.uma_runtime import UmaSpmdEngine

    s = diamond_si((6, 2, 2), jitter=0.2, seed=3)
    s.species = np.asarray(s.species) % 3
    cfg = UMAConfig(n_elements=3, sphere_channels=64, num_layers=2)
    core = UMACore.seeded(cfg, seed=1).float()
    return UmaSpmdEngine(core, world=1, threads=4, autocast_bf16=ac).step(s)


def _close(a, b, re, rf):
    e0, e1 = a["energy"].item(), b["energy"].item()
    assert abs(e0 - e1) < re * max(1.0, abs(e0)), (e0, e1)
    scale = a["forces_owned"].abs().max().item()
    dF = (a["forces_owned"] - b["forces_owned"]).abs().max().item()
    print(f"dF {dF:.3e} scale {scale:.3e}")
    assert dF < rf * max(1.0, scale), (dF, scale)


def test_so2_fused_engine(monkeypatch):
    """bf16 mode through the kernel stays within the bf16-autocast bounds of
    the fp32 engine, and so does DM_UMA_SO2=torch (the earlier path)."""
    f32, fused = _engine_step(False), _engine_step(True)
    _close(f32, fused, 2e-2, 5e-2)
    monkeypatch.setenv("DM_UMA_SO2", "torch")
    torch_bf16 = _engine_step(True)
    _close(f32, torch_bf16, 2e-2, 5e-2)
    assert not torch.equal(fused["forces_owned"], torch_bf16["forces_owned"])


def test_so2_fused_engine_chunked(monkeypatch):
    """A chunked pass through the kernel against the unchunked pass, at the
    tolerance of test_uma_engine_gpu_chunked_matches (1e-3 of the force
    scale, set for the fp32 engine).  Measured on MI355X: 0.0399 at force
    scale 44.8.  Chunking changes the order in which a source node's edge
    gradients are added in fp32, and the bf16 roundings after it turn that
    last bit into this difference."""
    ref = _engine_step(True)
    monkeypatch.setenv("DM_UMA_CHUNK", "3000")
    _close(ref, _engine_step(True), 1e-4, 1e-3)


def test_so2_fused_engine_bf16_repeats_bitwise():
    """bf16 mode through the kernel gives the same forces twice, bit for bit:
    the gather reverse is summed in a fixed order there (with atomic adds the
    bf16 roundings downstream moved the forces by 2e-3 of their scale)."""
    assert torch.equal(_engine_step(True)["forces_owned"],
                       _engine_step(True)["forces_owned"])


@pytest.mark.parametrize("ordered", [False, True])
def test_rot_gather_reverse_ordered(ordered):
    """_RotGather's dh and dD against the einsum composition in fp64, with
    the atomic and with the fixed-order sum; repeated node indices."""
    from distmlip_amd import so3, uma_ops

    gen = torch.Generator().manual_seed(5)
    dev = torch.device("cuda:0")
    N, E, C = 37, 301, 64
    h = torch.randn(N, 9, C, generator=gen).to(dev)
    R = so3.edge_align_rotation(torch.randn(E, 3, generator=gen).double())
    D = so3.wigner_D_batch(R, 2).float().to(dev)
    idx = torch.randint(0, N, (E,), generator=gen).int().to(dev)
    lw = torch.randn(E, 9, C, generator=gen).to(dev)

    def grads(fn, dt):
        a = [h.to(dt).requires_grad_(True), D.to(dt).requires_grad_(True)]
        return torch.autograd.grad((fn(*a) * lw.to(dt)).sum(), a)

    ref = grads(lambda h_, D_: torch.einsum("est,etc->esc", D_,
                                            h_[idx.long()]), torch.float64)
    got = grads(lambda h_, D_: uma_ops._RotGather.apply(h_, D_, idx, ordered),
                torch.float32)
    # fp32 sums of ~E/N = 8 (dh) and C = 64 (dD) terms of size <~ 10 and 30:
    # a few 1e-6; the bounds leave 10x
    assert (got[0].double() - ref[0]).abs().max().item() < 5e-5
    assert (got[1].double() - ref[1]).abs().max().item() < 3e-4
