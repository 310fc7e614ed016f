"""GPU tests of the fused gated-MLP reverse tail (k_gated_mlp_tail_bwd, entry
point dm_gated_mlp_tail_bwd_f32): tile tails, guard regions, accuracy
against fp64 relative to the three-kernel fp32 chain it replaces
(dm_gated_combine_bwd_f32, two GEMMs, dm_silu_bwd_f32), bitwise
repeatability, the d != 64 guard, gradients through gated_mlp_split3/4
(plain and under checkpoint), and the hand-sequenced conv reverse passes
with and without the new primitive.

The accuracy bound everywhere: max |err| against fp64 at most 2x that of
the three-kernel chain on the same inputs (two equally long fp32 fma chains
in different orders), the bound tests/test_gpu_edge_mlp_mfma.py uses."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs HIP GPU")

D = 64
GUARD = 256                 # floats on either side of dz / dw
SENTINEL = -12345.5
# Grid cap: 768 blocks of 4 waves, one 32-row tile per wave per iteration.
# 129*32+5 rows: 130 tiles in 33 blocks, ragged last tile, one tile per
# wave.  4097*32+5 rows: 4098 tiles > 3072 waves, so the first 1026 waves
# take a second tile and the rest do not; the last tile is ragged.
E_MULTI_BLOCK = 129 * 32 + 5
E_MULTI_TILE = 4097 * 32 + 5
E_CASES = [1, 31, 32, 33, 63, 64, 65, E_MULTI_BLOCK, E_MULTI_TILE]


def _f64_tail(go, c, g, w, z, w2):
    """fp64 torch evaluation of the formulas in include/distmlip_hip.h"""
    go, c, g, z, w2 = (t.double() for t in (go, c, g, z, w2))
    wv = w.double() if w is not None else 1.0
    sc, sg = torch.sigmoid(c), torch.sigmoid(g)
    silu_c = c * sc
    dc = go * wv * sg * (sc * (1 + c * (1 - sc)))
    dg = go * wv * silu_c * sg * (1 - sg)
    dw = go * silu_c * sg
    dh = torch.cat([dc @ w2[0].t(), dg @ w2[1].t()], dim=1)
    s = torch.sigmoid(z)
    return dh * (s * (1 + z * (1 - s))), dw


def _chain(go, cg, w, z, w2):
    """The three-kernel fp32 chain on the same inputs, (dz, dw): combine
    reverse, the two strided GEMMs of chgnet._SecondLayer.backward, SiLU
    reverse."""
    from distmlip_amd.ops import HipOps, raw_silu_bwd
    dcg, dw = HipOps().r_combine_bwd(go, cg, w)
    dh = torch.empty(go.shape[0], 2 * D, device=go.device)
    torch.mm(dcg[0], w2[0].t(), out=dh[:, :D])
    torch.mm(dcg[1], w2[1].t(), out=dh[:, D:])
    return raw_silu_bwd(dh, None, z), dw


class _Data:
    """One set of inputs of E_MULTI_TILE rows; every case uses a prefix.
    References are computed once and never modified."""

    def __init__(self):
        dev = torch.device("cuda:0")
        gen = torch.Generator(device="cpu").manual_seed(4321)
        E = E_MULTI_TILE
        self.dev = dev
        self.go = torch.randn(E, D, generator=gen).to(dev)
        self.cg = torch.randn(2, E, D, generator=gen).to(dev)
        self.w = torch.randn(E, D, generator=gen).to(dev)
        self.z = torch.randn(E, 2 * D, generator=gen).to(dev)
        self.w2 = (torch.randn(2, D, D, generator=gen) / 8).to(dev)
        self.ref = {}
        for has_w in (True, False):
            w = self.w if has_w else None
            dz64, dw64 = _f64_tail(self.go, self.cg[0], self.cg[1], w,
                                   self.z, self.w2)
            dz32, dw32 = _chain(self.go, self.cg, w, self.z, self.w2)
            self.ref[has_w] = (dz64, dw64, dz32, dw32)


@pytest.fixture(scope="module")
def data():
    return _Data()


def _fptr(t, off=0):
    return ctypes.cast(t.data_ptr() + 4 * off, ctypes.POINTER(ctypes.c_float))


def _launch(d, E, has_w, dim=D, expect_rc0=True):
    """Run the kernel through the C entry point into guarded buffers on the
    first E rows.  Returns (dz, dw or None, rc); asserts the guards."""
    from distmlip_amd.ops import _stream, hip_lib
    lib = hip_lib()
    cg = d.cg[:, :E].contiguous()
    go, z = d.go[:E], d.z[:E]
    w = d.w[:E] if has_w else None
    zbuf = torch.full((2 * GUARD + E * 2 * D,), SENTINEL, device=d.dev)
    wbuf = torch.full((2 * GUARD + E * D,), SENTINEL, device=d.dev)
    dz = zbuf[GUARD:GUARD + E * 2 * D].view(E, 2 * D)
    dw = wbuf[GUARD:GUARD + E * D].view(E, D)
    rc = lib.dm_gated_mlp_tail_bwd_f32(
        _fptr(go), _fptr(cg), _fptr(cg, E * D),
        _fptr(w) if has_w else None, _fptr(z), _fptr(d.w2),
        _fptr(d.w2, D * D), _fptr(dz), _fptr(dw) if has_w else None, E, dim,
        _stream())
    torch.cuda.synchronize()
    if not expect_rc0:
        assert rc != 0
        assert bool((zbuf == SENTINEL).all()) and bool((wbuf == SENTINEL).all())
        return None, None, rc
    assert rc == 0, lib.dm_hip_last_error()
    for name, buf, n in (("dz", zbuf, E * 2 * D), ("dw", wbuf, E * D)):
        assert bool((buf[:GUARD] == SENTINEL).all()), f"{name}: front guard"
        assert bool((buf[GUARD + n:] == SENTINEL).all()), \
            f"{name}: rear guard written (E={E})"
        if name == "dw" and not has_w:
            assert bool((buf == SENTINEL).all()), "dw written without w"
        else:
            assert not bool((buf[GUARD:GUARD + n] == SENTINEL).any()), \
                f"{name}: rows left unwritten (E={E})"
    return dz, (dw if has_w else None), rc


def _bound(got, ref64, chain, what):
    err = (got.double() - ref64).abs().max().item()
    err_chain = (chain.double() - ref64).abs().max().item()
    print(f"{what}: err fused {err:.3e} chain {err_chain:.3e}")
    assert err <= 2 * err_chain, \
        f"{what}: err fused {err:.3e} > 2 x chain {err_chain:.3e}"


@requires_gpu
@pytest.mark.parametrize("E", E_CASES)
@pytest.mark.parametrize("has_w", [True, False])
def test_tiles_tails_guards(data, has_w, E):
    d = data
    dz64, dw64, dz32, dw32 = (t[:E] if t is not None else None
                              for t in d.ref[has_w])
    dz, dw, _ = _launch(d, E, has_w)
    _bound(dz, dz64, dz32, f"dz w={has_w} E={E}")
    if has_w:
        _bound(dw, dw64, dw32, f"dw E={E}")
        print(f"dw E={E}: bitwise equal to k_gated_combine_bwd's: "
              f"{torch.equal(dw, dw32)}")
    dz2, dw2, _ = _launch(d, E, has_w)
    assert torch.equal(dz2, dz)
    if has_w:
        assert torch.equal(dw2, dw)


@requires_gpu
@pytest.mark.parametrize("dim", [32, 63, 65, 128])
def test_other_widths_refused(data, dim):
    _launch(data, 70, True, dim=dim, expect_rc0=False)


# --------------------------------------------------------------------------
# through autograd
# --------------------------------------------------------------------------
N_NODES, N_BONDS, E_SMALL = 50, 80, 1003


def _csr_of(idx64, n, dev):
    order = torch.argsort(idx64, stable=True)
    rp = torch.from_numpy(np.searchsorted(
        idx64[order].numpy(), np.arange(n + 1)).astype(np.int32)).to(dev)
    return order.to(torch.int32).to(dev), rp


class _PD:
    pass


def _graphs(dev):
    """(pd for HipOps with int32 indices and CSRs, pd for the plain-torch
    reference with int64 indices): E_SMALL edges over N_NODES atoms and
    E_SMALL lines over N_BONDS bonds."""
    gen = torch.Generator(device="cpu").manual_seed(77)
    E, N, B = E_SMALL, N_NODES, N_BONDS
    src = torch.randint(0, N, (E,), generator=gen)
    dst = torch.sort(torch.randint(0, N, (E,), generator=gen)).values
    l_src = torch.randint(0, B, (E,), generator=gen)
    l_dst = torch.sort(torch.randint(0, B, (E,), generator=gen)).values
    center = torch.randint(0, N, (E,), generator=gen)
    pd, pr = _PD(), _PD()
    for p in (pd, pr):
        p.n_atoms, p.n_bonds = N, B
    for name, t in (("src", src), ("dst", dst), ("l_src", l_src),
                    ("l_dst", l_dst), ("center", center)):
        setattr(pd, name, t.to(torch.int32).to(dev))
        setattr(pr, name, t.to(dev))
    pd.src_perm, pd.src_row_ptr = _csr_of(src, N, dev)
    _, pd.row_ptr = _csr_of(dst, N, dev)
    pd.line_src_perm, pd.line_src_row_ptr = _csr_of(l_src, B, dev)
    _, pd.line_row_ptr = _csr_of(l_dst, B, dev)
    pd.center_perm, pd.center_row_ptr = _csr_of(center, N, dev)
    return pd, pr


def _mlp(in_mult, dev, seed):
    from distmlip_amd.model import GatedMLP
    torch.manual_seed(seed)
    mlp = GatedMLP(in_mult * D, D, D).to(dev)
    for p in mlp.parameters():
        p.requires_grad_(False)
    return mlp


@pytest.fixture(scope="module")
def graphs():
    return _graphs(torch.device("cuda:0"))


def _leaves(ts, dtype=torch.float32):
    return [t.detach().to(dtype).clone().requires_grad_(True) if t is not None
            else None for t in ts]


def _grads(fn, leaves, go):
    out = fn(*leaves)
    out.backward(go.to(out.dtype))
    return [t.grad for t in leaves if t is not None]


def _autograd_case(monkeypatch, graphs, kind, with_w, with_base, ckpt=False):
    """Gradients of one gated_mlp_split call: fused tail, the same call
    under DM_NO_FUSED_MLP_BWD=1, and fp64 plain torch."""
    import copy

    from distmlip_amd.chgnet import gated_mlp_split3, gated_mlp_split4
    from distmlip_amd.ops import HipOps
    from oracle.chgnet_ref import CpuRefOps
    pd, pr = graphs
    dev = pd.src.device
    gen = torch.Generator(device="cpu").manual_seed(5 + 2 * with_w + with_base)
    mlp = _mlp(3 if kind == 3 else 4, dev, seed=11 + kind)
    mlp64 = copy.deepcopy(mlp).double()
    v = torch.randn(N_NODES, D, generator=gen).to(dev)
    e = torch.randn(E_SMALL, D, generator=gen).to(dev)
    n = torch.randn(N_BONDS, D, generator=gen).to(dev)
    w = torch.randn(E_SMALL, D, generator=gen).to(dev) if with_w else None
    go = torch.randn(E_SMALL, D, generator=gen).to(dev)

    def call(ops, m, p):
        if kind == 3:
            def fn(e_, v_, w_):
                return gated_mlp_split3(m, v_, e_, p, ops, D, w=w_,
                                        base=e_ if with_base else None)
            return fn, (e, v, w)

        def fn(a_, n_, v_, w_):
            return gated_mlp_split4(m, n_, a_, v_, p, ops, D, w=w_,
                                    base=a_ if with_base else None)
        return fn, (e, n, v, w)

    def run(ops, m, p, dtype=torch.float32):
        fn, ins = call(ops, m, p)
        if ckpt:
            inner = fn

            def fn(*a):
                return torch.utils.checkpoint.checkpoint(
                    inner, *a, use_reentrant=False)
        return _grads(fn, _leaves(ins, dtype), go)

    launches = []
    import distmlip_amd.ops as ops_mod
    real = ops_mod.raw_mlp_tail_bwd
    monkeypatch.setattr(ops_mod, "raw_mlp_tail_bwd",
                        lambda *a: (launches.append(1), real(*a))[1])
    monkeypatch.delenv("DM_NO_FUSED_MLP_BWD", raising=False)
    fused = run(HipOps(), mlp, pd)
    assert len(launches) == 1, "the fused tail kernel did not run"
    monkeypatch.setenv("DM_NO_FUSED_MLP_BWD", "1")
    chain = run(HipOps(), mlp, pd)
    assert len(launches) == 1, "DM_NO_FUSED_MLP_BWD=1 still ran the kernel"
    ref = run(CpuRefOps(), mlp64, pr, torch.float64)
    assert len(fused) == len(chain) == len(ref)
    for i, (f, c, r) in enumerate(zip(fused, chain, ref)):
        _bound(f, r, c, f"split{kind} w={with_w} base={with_base} "
                        f"ckpt={ckpt} grad[{i}]")
    return fused


@requires_gpu
@pytest.mark.parametrize("kind,with_w,with_base", [
    (3, True, True), (3, True, False), (4, True, False), (4, False, True)])
def test_autograd(monkeypatch, graphs, kind, with_w, with_base):
    _autograd_case(monkeypatch, graphs, kind, with_w, with_base)


@requires_gpu
def test_autograd_checkpoint(monkeypatch, graphs):
    """Under non-reentrant checkpointing, as runtime.py runs the blocks,
    the gradients are those of the plain call bit for bit."""
    ck = _autograd_case(monkeypatch, graphs, 3, True, True, ckpt=True)
    plain = _autograd_case(monkeypatch, graphs, 3, True, True)
    for a, b in zip(ck, plain):
        assert torch.equal(a, b)


@requires_gpu
def test_mlp_tail_rejects_foreign_h(graphs):
    """z and h from two different first-layer calls are refused."""
    from distmlip_amd.ops import HipOps
    pd, _ = graphs
    dev = pd.src.device
    ops = HipOps()
    zs = torch.randn(N_NODES, 2 * D, device=dev, requires_grad=True)
    ze = torch.randn(E_SMALL, 2 * D, device=dev)
    z1, _h1 = ops.gather_add3_zh(zs, zs, ze, pd)
    _z2, h2 = ops.gather_add3_zh(zs, zs, ze, pd)
    w2 = torch.randn(2, D, D, device=dev)
    b2 = torch.zeros(2, 1, D, device=dev)
    with pytest.raises(AssertionError):
        ops.mlp_tail(z1, h2, w2, b2)


# --------------------------------------------------------------------------
# hand-sequenced conv reverse passes, with and without the primitive
# --------------------------------------------------------------------------
def _packs(mlp):
    from distmlip_amd.chgnet import _packed_weights
    return _packed_weights(mlp)[:4]


def _conv_compare(monkeypatch, run):
    """run(ops, dtype, ref) -> tuple of tensors; fused vs chain vs fp64"""
    from distmlip_amd.ops import HipOps
    from oracle.chgnet_ref import CpuRefOps
    monkeypatch.delenv("DM_NO_FUSED_MLP_BWD", raising=False)
    fused = run(HipOps(), torch.float32, False)
    monkeypatch.setenv("DM_NO_FUSED_MLP_BWD", "1")
    chain = run(HipOps(), torch.float32, False)
    ref = run(CpuRefOps(), torch.float64, True)
    for i, (f, c, r) in enumerate(zip(fused, chain, ref)):
        _bound(f, r, c, f"out[{i}]")


@requires_gpu
def test_conv_parity(monkeypatch, graphs):
    from distmlip_amd import conv
    pd, pr = graphs
    dev = pd.src.device
    gen = torch.Generator(device="cpu").manual_seed(31)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen).to(dev)

    v, e, n = rnd(N_NODES, D), rnd(E_SMALL, D), rnd(N_BONDS, D)
    wbb, wab, w3 = rnd(E_SMALL, D), rnd(E_SMALL, D), rnd(N_BONDS, D)
    go_v, go_e, go_n = rnd(N_NODES, D), rnd(E_SMALL, D), rnd(N_BONDS, D)
    m_e, m_n = _mlp(3, dev, 1), _mlp(3, dev, 2)
    m_b, m_a = _mlp(4, dev, 3), _mlp(4, dev, 4)

    def packs(m, dtype):
        import copy
        return _packs(copy.deepcopy(m).to(dtype))

    def atom(ops, dtype, ref):
        p = pr if ref else pd
        t = [x.to(dtype) for x in (v, e, wbb, wab, go_v, go_e)]
        pe, pn = packs(m_e, dtype), packs(m_n, dtype)
        _, _, saved = conv.atom_fwd(ops, p, t[0], t[1], t[2], t[3], pe, pn, D)
        return conv.atom_bwd(ops, p, saved, pe, pn, D, t[2], t[3], t[4], t[5])

    def bond(ops, dtype, ref):
        p = pr if ref else pd
        t = [x.to(dtype) for x in (n, e, v, w3, go_n)]
        pb = packs(m_b, dtype)
        _, saved = conv.bond_fwd(ops, p, t[0], t[1], t[2], t[3], pb, D)
        return conv.bond_bwd(ops, p, saved, pb, D, t[4])

    def angle(ops, dtype, ref):
        p = pr if ref else pd
        t = [x.to(dtype) for x in (n, e, v, go_e)]
        pa = packs(m_a, dtype)
        _, saved = conv.angle_fwd(ops, p, t[0], t[1], t[2], pa, D)
        return conv.angle_bwd(ops, p, saved, pa, D, t[3])

    calls = []
    from distmlip_amd.ops import HipOps
    real = HipOps.r_mlp_tail_bwd
    monkeypatch.setattr(HipOps, "r_mlp_tail_bwd",
                        lambda self, *a: (calls.append(1), real(self, *a))[1])
    for run, n_mlps in ((atom, 2), (bond, 1), (angle, 1)):
        del calls[:]
        _conv_compare(monkeypatch, run)
        assert len(calls) == n_mlps, "the fused primitive was not used"
