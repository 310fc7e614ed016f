"""GPU tests of the fp32-MFMA fused first-layer edge-MLP kernel
(k_edge_mlp_64x128<2|3>, entry points dm_edge_mlp3_f32 / dm_edge_mlp4_f32):
tile tails, guard regions, index extremes, accuracy against fp64 relative
to the unfused fp32 path, bitwise consistency, and gradients through
_EdgeMlp3 / _EdgeMlp4."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs HIP GPU")

DIN, DOUT = 64, 128
N_NODES = 50
GUARD = 256                 # floats on either side of z / h
SENTINEL = -12345.5
# The launch is capped at 768 blocks of 4 waves, one 32-row tile per wave
# per iteration, so a wave only loops over a second tile when there are more
# than 3072 tiles.  129*32+5 rows (the size the issue names) gives 130 tiles
# in 33 blocks: more than one block, a ragged last tile, one tile per wave.
# 4097*32+5 rows lies beyond the cap: the first 1026 waves take a second
# tile, the rest do not, and the very last tile is ragged.
E_MULTI_BLOCK = 129 * 32 + 5
E_MULTI_TILE = 4097 * 32 + 5
E_CASES = [1, 31, 32, 33, 63, 64, 65, E_MULTI_BLOCK, E_MULTI_TILE]


class _Data:
    """One set of inputs of E_MULTI_TILE rows; every case uses a prefix.
    References are computed once and never modified."""

    def __init__(self):
        dev = torch.device("cuda:0")
        g = torch.Generator(device="cpu").manual_seed(1234)
        E = E_MULTI_TILE
        self.dev = dev
        self.erow = torch.randn(E, DIN, generator=g).to(dev)
        self.wt = torch.randn(DIN, DOUT, generator=g).to(dev)
        self.bias = torch.randn(DOUT, generator=g).to(dev)
        self.g = [torch.randn(N_NODES, DOUT, generator=g).to(dev)
                  for _ in range(3)]
        self.idx = [torch.randint(0, N_NODES, (E,), generator=g)
                    .to(torch.int32).to(dev) for _ in range(3)]
        self.ref = {ng: self.reference(ng, self.erow, self.idx)
                    for ng in (2, 3)}

    def reference(self, ng, erow, idx):
        """(z fp64, z unfused fp32, h unfused fp32) for the first ng gathers"""
        li = [i.long() for i in idx[:ng]]
        z64 = erow.double() @ self.wt.double() + self.bias.double()
        z32 = erow @ self.wt + self.bias
        for t, i in zip(self.g[:ng], li):
            z64 = z64 + t.double()[i]
            z32 = z32 + t[i]
        return z64, z32, torch.nn.functional.silu(z32)


@pytest.fixture(scope="module")
def data():
    return _Data()


def _launch(d, ng, E, erow, idx, store_z):
    """Run the kernel through the C entry point into guarded buffers.
    Returns (z or None, h); asserts the guards are untouched."""
    from distmlip_amd.ops import _fp, _ip, _stream, hip_lib
    lib = hip_lib()

    def guarded():
        return torch.full((2 * GUARD + E * DOUT,), SENTINEL, device=d.dev)

    hbuf = guarded()
    zbuf = guarded() if store_z else None
    h = hbuf[GUARD:GUARD + E * DOUT].view(E, DOUT)
    z = zbuf[GUARD:GUARD + E * DOUT].view(E, DOUT) if store_z else None
    zp = _fp(z) if store_z else None
    if ng == 2:
        rc = lib.dm_edge_mlp3_f32(
            _fp(erow), _fp(d.wt), _fp(d.bias), _fp(d.g[0]), _fp(d.g[1]),
            _ip(idx[0]), _ip(idx[1]), zp, _fp(h), E, DIN, DOUT, _stream())
    else:
        rc = lib.dm_edge_mlp4_f32(
            _fp(erow), _fp(d.wt), _fp(d.bias), _fp(d.g[0]), _fp(d.g[1]),
            _fp(d.g[2]), _ip(idx[0]), _ip(idx[1]), _ip(idx[2]), zp, _fp(h),
            E, DIN, DOUT, _stream())
    assert rc == 0, lib.dm_hip_last_error()
    torch.cuda.synchronize()
    for name, buf in (("h", hbuf), ("z", zbuf)):
        if buf is None:
            continue
        assert bool((buf[:GUARD] == SENTINEL).all()), f"{name}: front guard"
        assert bool((buf[GUARD + E * DOUT:] == SENTINEL).all()), \
            f"{name}: rear guard written (E={E})"
        assert not bool((buf[GUARD:GUARD + E * DOUT] == SENTINEL).any()), \
            f"{name}: rows left unwritten (E={E})"
    return z, h


def _check_accuracy(z, h, z64, z32, h32, what):
    """max |err| vs fp64 at most 2x the unfused fp32 path's on the same
    inputs (an equally long fp32 fma chain in another order)."""
    h64 = torch.nn.functional.silu(z64)
    if z is not None:
        err = (z.double() - z64).abs().max().item()
        err_unf = (z32.double() - z64).abs().max().item()
        print(f"{what}: z err fused {err:.3e} unfused {err_unf:.3e}")
        assert err <= 2 * err_unf, \
            f"{what}: z err fused {err:.3e} > 2 x unfused {err_unf:.3e}"
    err = (h.double() - h64).abs().max().item()
    err_unf = (h32.double() - h64).abs().max().item()
    print(f"{what}: h err fused {err:.3e} unfused {err_unf:.3e}")
    assert err <= 2 * err_unf, \
        f"{what}: h err fused {err:.3e} > 2 x unfused {err_unf:.3e}"


@requires_gpu
@pytest.mark.parametrize("E", E_CASES)
@pytest.mark.parametrize("ng", [2, 3])
def test_tiles_tails_guards(data, ng, E):
    d = data
    erow = d.erow[:E]
    idx = [i[:E] for i in d.idx]
    z64, z32, h32 = (t[:E] for t in d.ref[ng])
    z, h = _launch(d, ng, E, erow, idx, store_z=True)
    _check_accuracy(z, h, z64, z32, h32, f"<{ng}> E={E}")
    # no-z launch: same h bit for bit, accuracy bound holds on its own
    _, h_noz = _launch(d, ng, E, erow, idx, store_z=False)
    assert torch.equal(h_noz, h), "h differs between no-z and z launches"
    _check_accuracy(None, h_noz, z64, z32, h32, f"<{ng}> E={E} no-z")
    # identical launches are bit-identical
    z2, h2 = _launch(d, ng, E, erow, idx, store_z=True)
    assert torch.equal(z2, z) and torch.equal(h2, h)


@requires_gpu
@pytest.mark.parametrize("ng", [2, 3])
@pytest.mark.parametrize("case", ["same_dst", "all_zero", "all_last",
                                  "duplicates", "ends_mixed"])
def test_index_extremes(data, ng, case):
    d = data
    E = 3 * 32 + 7
    erow = d.erow[:E]
    ar = torch.arange(E)
    src, dst, ctr = (i[:E].cpu().long() for i in d.idx)
    if case == "same_dst":
        dst = torch.full((E,), 17)
    elif case == "all_zero":
        src = dst = ctr = torch.zeros(E, dtype=torch.long)
    elif case == "all_last":
        src = dst = ctr = torch.full((E,), N_NODES - 1)
    elif case == "duplicates":
        src, dst, ctr = ar % 3, (ar // 2) % 5, ar % 2
    else:
        src = (ar % 2) * (N_NODES - 1)
        dst = ((ar + 1) % 2) * (N_NODES - 1)
        ctr = ((ar // 32) % 2) * (N_NODES - 1)
    idx = [t.to(torch.int32).to(d.dev) for t in (src, dst, ctr)]
    z64, z32, h32 = d.reference(ng, erow, idx)
    for store_z in (True, False):
        z, h = _launch(d, ng, E, erow, idx, store_z)
        _check_accuracy(z, h, z64, z32, h32, f"<{ng}> {case} z={store_z}")


def _csr_of(idx64, n, dev):
    order = torch.argsort(idx64, stable=True)
    rp = torch.from_numpy(np.searchsorted(
        idx64[order].numpy(), np.arange(n + 1)).astype(np.int32)).to(dev)
    return order.to(torch.int32).to(dev), rp


@requires_gpu
@pytest.mark.parametrize("E", [33, 2000])
def test_gradients(data, E):
    """Backward of _EdgeMlp3/_EdgeMlp4 (unchanged code, consumes the saved
    z) against autograd of the fp32 torch expression; tolerances of
    tests/test_gpu.py::test_edge_mlp_fused_vs_unfused."""
    from distmlip_amd.ops import _EdgeMlp3, _EdgeMlp4
    d, dev = data, data.dev
    gen = torch.Generator(device="cpu").manual_seed(99 + E)
    N, B = N_NODES, 80

    def leaf(t):
        return t.detach().clone().requires_grad_(True)

    src64 = torch.randint(0, N, (E,), generator=gen)
    dst64 = torch.sort(torch.randint(0, N, (E,), generator=gen)).values
    sperm, srp = _csr_of(src64, N, dev)
    _, drp = _csr_of(dst64, N, dev)
    erow, zs, zd = leaf(d.erow[:E]), leaf(d.g[0]), leaf(d.g[1])
    z, h = _EdgeMlp3.apply(erow, d.wt, d.bias, zs, zd,
                           src64.to(torch.int32).to(dev),
                           dst64.to(torch.int32).to(dev), sperm, srp, drp)
    e2, zs2, zd2 = leaf(erow), leaf(zs), leaf(zd)
    zref = e2 @ d.wt + d.bias + zs2[src64.to(dev)] + zd2[dst64.to(dev)]
    href = torch.nn.functional.silu(zref)
    assert torch.allclose(z, zref, atol=2e-4), (z - zref).abs().max()
    assert torch.allclose(h, href, atol=2e-4)
    go = torch.randn(E, DOUT, generator=gen).to(dev)
    h.backward(go)
    href.backward(go)
    assert torch.allclose(erow.grad, e2.grad, atol=2e-3), \
        (erow.grad - e2.grad).abs().max()
    assert torch.allclose(zs.grad, zs2.grad, atol=2e-3)
    assert torch.allclose(zd.grad, zd2.grad, atol=2e-3)

    class PD:
        pass
    l_src64 = torch.randint(0, B, (E,), generator=gen)
    l_dst64 = torch.sort(torch.randint(0, B, (E,), generator=gen)).values
    c64 = torch.randint(0, N, (E,), generator=gen)
    pd = PD()
    pd.l_src = l_src64.to(torch.int32).to(dev)
    pd.l_dst = l_dst64.to(torch.int32).to(dev)
    pd.center = c64.to(torch.int32).to(dev)
    pd.line_src_perm, pd.line_src_row_ptr = _csr_of(l_src64, B, dev)
    _, pd.line_row_ptr = _csr_of(l_dst64, B, dev)
    pd.center_perm, pd.center_row_ptr = _csr_of(c64, N, dev)
    a = leaf(d.erow[E:2 * E])
    z1 = leaf(torch.randn(B, DOUT, generator=gen).to(dev))
    z2 = leaf(torch.randn(B, DOUT, generator=gen).to(dev))
    zv = leaf(d.g[2])
    z, h = _EdgeMlp4.apply(a, d.wt, d.bias, z1, z2, zv, pd)
    a2, z12, z22, zv2 = leaf(a), leaf(z1), leaf(z2), leaf(zv)
    zref = (a2 @ d.wt + d.bias + z12[l_src64.to(dev)] + z22[l_dst64.to(dev)]
            + zv2[c64.to(dev)])
    href = torch.nn.functional.silu(zref)
    assert torch.allclose(z, zref, atol=2e-4), (z - zref).abs().max()
    assert torch.allclose(h, href, atol=2e-4)
    h.backward(go)
    href.backward(go)
    assert torch.allclose(a.grad, a2.grad, atol=2e-3), \
        (a.grad - a2.grad).abs().max()
    assert torch.allclose(z1.grad, z12.grad, atol=2e-3)
    assert torch.allclose(z2.grad, z22.grad, atol=2e-3)
    assert torch.allclose(zv.grad, zv2.grad, atol=2e-3)
