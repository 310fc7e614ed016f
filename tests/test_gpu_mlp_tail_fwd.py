"""GPU tests of the fused gated-MLP forward tail (k_gated_mlp_tail_fwd, entry
point dm_gated_mlp_tail_fwd_f32): tile tails, guard regions, every
keep-cg x w x base variant, accuracy against fp64 relative to the fp32 chain
it replaces (torch.baddbmm + dm_gated_combine_fwd_f32), bitwise repeatability
and keep/no-keep identity, the refusals, gated_mlp_split3/4 through autograd
(plain, under no_grad and under checkpoint), and the hand-sequenced conv
passes with and without the new primitive.

The accuracy bound everywhere: max |err| against fp64 at most 2x that of
the chain on the same inputs (two equally long fp32 fma chains in different
orders), the bound tests/test_gpu_edge_mlp_mfma.py and
tests/test_gpu_mlp_tail_bwd.py use."""
import copy
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs HIP GPU")

D = 64
GUARD = 256                 # floats on either side of c / g / out
SENTINEL = -12345.5
# Grid cap: 768 blocks of 4 waves, one 32-row tile per wave per iteration.
# 129*32+5 rows: 130 tiles in 33 blocks, ragged last tile, one tile per
# wave.  4097*32+5 rows: 4098 tiles > 3072 waves, so the first 1026 waves
# take a second tile and the rest do not; the last tile is ragged.
E_MULTI_BLOCK = 129 * 32 + 5
E_MULTI_TILE = 4097 * 32 + 5
E_CASES = [1, 31, 32, 33, 63, 64, 65, E_MULTI_BLOCK, E_MULTI_TILE]


def _f64_tail(cg64, w, base):
    c, g = cg64[0], cg64[1]
    out = c * torch.sigmoid(c) * torch.sigmoid(g)
    if w is not None:
        out = out * w.double()
    if base is not None:
        out = out + base.double()
    return out


class _Data:
    """One set of inputs of E_MULTI_TILE rows; every case uses a prefix.
    References are computed once and never modified."""

    def __init__(self):
        from distmlip_amd.ops import HipOps
        dev = torch.device("cuda:0")
        gen = torch.Generator(device="cpu").manual_seed(8765)
        E = E_MULTI_TILE
        self.dev = dev
        self.h = torch.nn.functional.silu(
            torch.randn(E, 2 * D, generator=gen)).to(dev)
        self.w2 = (torch.randn(2, D, D, generator=gen) / 8).to(dev)
        self.b2 = torch.randn(2, 1, D, generator=gen).to(dev)
        self.w = torch.randn(E, D, generator=gen).to(dev)
        self.base = torch.randn(E, D, generator=gen).to(dev)
        hb = self.h.view(-1, 2, D).transpose(0, 1)
        self.cg64 = torch.baddbmm(self.b2.double(), hb.double(),
                                  self.w2.double())
        self.cg32 = torch.baddbmm(self.b2, hb, self.w2)
        self.out = {}
        for has_w in (True, False):
            for has_base in (True, False):
                w = self.w if has_w else None
                base = self.base if has_base else None
                self.out[has_w, has_base] = (
                    _f64_tail(self.cg64, w, base),
                    HipOps().r_combine_fwd(self.cg32, w, base))


@pytest.fixture(scope="module")
def data():
    return _Data()


def _fptr(t, off=0):
    return ctypes.cast(t.data_ptr() + 4 * off, ctypes.POINTER(ctypes.c_float))


def _launch(d, E, keep, has_w, has_base, dim=D, expect_rc0=True,
            only_one=None):
    """Run the kernel through the C entry point into guarded buffers on the
    first E rows.  Returns (c, g, out), c and g None without keep; asserts
    the guards.  only_one = "c" / "g" passes that pointer alone."""
    from distmlip_amd.ops import _stream, hip_lib
    lib = hip_lib()
    n = E * D
    bufs = [torch.full((2 * GUARD + n,), SENTINEL, device=d.dev)
            for _ in range(3)]
    c, g, out = (b[GUARD:GUARD + n].view(E, D) for b in bufs)
    cp = _fptr(c) if (keep and only_one != "g") else None
    gp = _fptr(g) if (keep and only_one != "c") else None
    rc = lib.dm_gated_mlp_tail_fwd_f32(
        _fptr(d.h), _fptr(d.w2), _fptr(d.w2, D * D), _fptr(d.b2),
        _fptr(d.b2, D), _fptr(d.w) if has_w else None,
        _fptr(d.base) if has_base else None, cp, gp, _fptr(out), E, dim,
        _stream())
    torch.cuda.synchronize()
    if not expect_rc0:
        assert rc != 0
        for b in bufs:
            assert bool((b == SENTINEL).all()), "a refused call wrote"
        return None, None, None
    assert rc == 0, lib.dm_hip_last_error()
    for name, buf in zip(("c", "g", "out"), bufs):
        assert bool((buf[:GUARD] == SENTINEL).all()), f"{name}: front guard"
        assert bool((buf[GUARD + n:] == SENTINEL).all()), \
            f"{name}: rear guard written (E={E})"
        if name != "out" and not keep:
            assert bool((buf == SENTINEL).all()), \
                f"{name} written in the no-keep form"
        else:
            assert not bool((buf[GUARD:] == SENTINEL)[:n].any()), \
                f"{name}: rows left unwritten (E={E})"
    return (c, g, out) if keep else (None, None, out)


def _bound(got, ref64, chain, what):
    err = (got.double() - ref64).abs().max().item()
    err_chain = (chain.double() - ref64).abs().max().item()
    print(f"{what}: err fused {err:.3e} chain {err_chain:.3e}")
    assert err <= 2 * err_chain, \
        f"{what}: err fused {err:.3e} > 2 x chain {err_chain:.3e}"


@requires_gpu
@pytest.mark.parametrize("E", E_CASES)
@pytest.mark.parametrize("has_base", [True, False])
@pytest.mark.parametrize("has_w", [True, False])
def test_tiles_tails_guards(data, has_w, has_base, E):
    """Both keep forms of one (w, base, E) case: guards, accuracy, a second
    launch, and out of the keep form against out of the no-keep form."""
    from distmlip_amd.ops import HipOps
    d = data
    out64, out32 = (t[:E] for t in d.out[has_w, has_base])
    tag = f"w={has_w} base={has_base} E={E}"
    c, g, out_k = _launch(d, E, True, has_w, has_base)
    _, _, out_n = _launch(d, E, False, has_w, has_base)
    cg = torch.stack([c, g])
    _bound(cg, d.cg64[:, :E], d.cg32[:, :E], f"cg {tag}")
    print(f"cg {tag}: bitwise equal to torch.baddbmm's: "
          f"{torch.equal(cg, d.cg32[:, :E])}")
    _bound(out_k, out64, out32, f"out {tag}")
    assert torch.equal(out_k, out_n), "out differs between keep and no-keep"
    c2, g2, out_k2 = _launch(d, E, True, has_w, has_base)
    assert torch.equal(c2, c) and torch.equal(g2, g)
    assert torch.equal(out_k2, out_k)
    _, _, out_n2 = _launch(d, E, False, has_w, has_base)
    assert torch.equal(out_n2, out_n)
    own = HipOps().r_combine_fwd(cg.contiguous(),
                                 d.w[:E] if has_w else None,
                                 d.base[:E] if has_base else None)
    print(f"out {tag}: bitwise equal to k_gated_combine_fwd over the "
          f"kernel's own cg: {torch.equal(own, out_k)}")


@requires_gpu
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("dim", [32, 63, 65, 128])
def test_other_widths_refused(data, dim, keep):
    _launch(data, 70, keep, True, True, dim=dim, expect_rc0=False)


@requires_gpu
@pytest.mark.parametrize("only_one", ["c", "g"])
def test_mixed_cg_pair_refused(data, only_one):
    _launch(data, 70, True, True, True, expect_rc0=False, only_one=only_one)


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
    """The small graph of tests/test_gpu_mlp_tail_bwd.py: (pd for HipOps
    with int32 indices and CSRs, pd for the plain-torch reference with
    int64 indices), E_SMALL edges over N_NODES atoms and E_SMALL lines over
    N_BONDS bonds."""
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


def _count_launches(monkeypatch):
    """Wrap ops.raw_mlp_tail_fwd; returns the list its launches append to."""
    import distmlip_amd.ops as ops_mod
    launches = []
    real = ops_mod.raw_mlp_tail_fwd
    monkeypatch.setattr(ops_mod, "raw_mlp_tail_fwd",
                        lambda *a: (launches.append(a[-1]), real(*a))[1])
    return launches


def _autograd_case(monkeypatch, graphs, kind, with_w, with_base, ckpt=False):
    """Output and input gradients of one gated_mlp_split call on three
    paths: default, DM_NO_FUSED_MLP_FWD=1 and fp64 plain torch.  Returns
    the default path's [out, grads...]."""
    from distmlip_amd.chgnet import gated_mlp_split3, gated_mlp_split4
    from distmlip_amd.ops import HipOps
    from oracle.chgnet_ref import CpuRefOps
    pd, pr = graphs
    dev = pd.src.device
    gen = torch.Generator(device="cpu").manual_seed(9 + 2 * with_w + with_base)
    mlp = _mlp(3 if kind == 3 else 4, dev, seed=21 + kind)
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
        leaves = _leaves(ins, dtype)
        out = fn(*leaves)
        out.backward(go.to(out.dtype))
        return [out.detach()] + [t.grad for t in leaves if t is not None]

    launches = _count_launches(monkeypatch)
    monkeypatch.delenv("DM_NO_FUSED_MLP_FWD", raising=False)
    fused = run(HipOps(), mlp, pd)
    # one recording launch per pass over the MLP; under a non-reentrant
    # checkpoint the outer forward records too (its saves are dropped by
    # the checkpoint's hooks), then the recomputation
    assert launches == ([True, True] if ckpt else [True]), launches
    if not ckpt:
        fn, ins = call(HipOps(), mlp, pd)
        with torch.no_grad():
            quiet = fn(*ins)
        assert launches == [True, False], "no_grad call: not the no-cg form"
        assert torch.equal(quiet, fused[0]), \
            "no_grad output differs from the recording call's"
    del launches[:]
    monkeypatch.setenv("DM_NO_FUSED_MLP_FWD", "1")
    chain = run(HipOps(), mlp, pd)
    with torch.no_grad():
        fn, ins = call(HipOps(), mlp, pd)
        fn(*ins)
    assert launches == [], "DM_NO_FUSED_MLP_FWD=1 still ran the kernel"
    monkeypatch.delenv("DM_NO_FUSED_MLP_FWD")
    ref = run(CpuRefOps(), mlp64, pr, torch.float64)
    assert launches == []
    assert len(fused) == len(chain) == len(ref)
    for i, (f, c, r) in enumerate(zip(fused, chain, ref)):
        _bound(f, r, c, f"split{kind} w={with_w} base={with_base} "
                        f"ckpt={ckpt} {'out' if i == 0 else f'grad[{i - 1}]'}")
    return fused


@requires_gpu
@pytest.mark.parametrize("kind,with_w,with_base", [
    (3, True, True), (3, False, False), (4, True, False), (4, False, True)])
def test_autograd(monkeypatch, graphs, kind, with_w, with_base):
    _autograd_case(monkeypatch, graphs, kind, with_w, with_base)


@requires_gpu
def test_autograd_checkpoint(monkeypatch, graphs):
    """Under non-reentrant checkpointing, as runtime.py runs the blocks, the
    output and the gradients are those of the plain call bit for bit."""
    ck = _autograd_case(monkeypatch, graphs, 3, True, True, ckpt=True)
    plain = _autograd_case(monkeypatch, graphs, 3, True, True)
    for a, b in zip(ck, plain):
        assert torch.equal(a, b)


@requires_gpu
def test_mlp_tail_act_refuses_recording(data):
    """The no-grad form does not silently drop a gradient."""
    from distmlip_amd.ops import HipOps
    d = data
    w = d.w[:70].clone().requires_grad_(True)
    with pytest.raises(AssertionError):
        HipOps().mlp_tail_act(d.h[:70], d.w2, d.b2, w)


# --------------------------------------------------------------------------
# hand-sequenced conv passes, with and without the primitive
# --------------------------------------------------------------------------
def _packs(mlp):
    from distmlip_amd.chgnet import _packed_weights
    return _packed_weights(mlp)[:4]


@requires_gpu
def test_conv_parity(monkeypatch, graphs):
    from distmlip_amd import conv
    from distmlip_amd.ops import HipOps
    from oracle.chgnet_ref import CpuRefOps
    pd, pr = graphs
    dev = pd.src.device
    gen = torch.Generator(device="cpu").manual_seed(41)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen).to(dev)

    v, e, n = rnd(N_NODES, D), rnd(E_SMALL, D), rnd(N_BONDS, D)
    wbb, wab, w3 = rnd(E_SMALL, D), rnd(E_SMALL, D), rnd(N_BONDS, D)
    go_v, go_e, go_n = rnd(N_NODES, D), rnd(E_SMALL, D), rnd(N_BONDS, D)
    m_e, m_n = _mlp(3, dev, 1), _mlp(3, dev, 2)
    m_b, m_a = _mlp(4, dev, 3), _mlp(4, dev, 4)

    def packs(m, dtype):
        return _packs(copy.deepcopy(m).to(dtype))

    def atom(ops, dtype, ref):
        p = pr if ref else pd
        t = [x.to(dtype) for x in (v, e, wbb, wab, go_v, go_e)]
        pe, pn = packs(m_e, dtype), packs(m_n, dtype)
        v2, e2, saved = conv.atom_fwd(ops, p, t[0], t[1], t[2], t[3], pe, pn,
                                      D)
        return (v2, e2) + tuple(conv.atom_bwd(
            ops, p, saved, pe, pn, D, t[2], t[3], t[4], t[5]))

    def bond(ops, dtype, ref):
        p = pr if ref else pd
        t = [x.to(dtype) for x in (n, e, v, w3, go_n)]
        pb = packs(m_b, dtype)
        n2, saved = conv.bond_fwd(ops, p, t[0], t[1], t[2], t[3], pb, D)
        return (n2,) + tuple(conv.bond_bwd(ops, p, saved, pb, D, t[4]))

    def angle(ops, dtype, ref):
        p = pr if ref else pd
        t = [x.to(dtype) for x in (n, e, v, go_e)]
        pa = packs(m_a, dtype)
        a2, saved = conv.angle_fwd(ops, p, t[0], t[1], t[2], pa, D)
        return (a2,) + tuple(conv.angle_bwd(ops, p, saved, pa, D, t[3]))

    calls = []
    real = HipOps.r_mlp_tail_fwd
    monkeypatch.setattr(HipOps, "r_mlp_tail_fwd",
                        lambda self, *a: (calls.append(1), real(self, *a))[1])
    for run, n_mlps in ((atom, 2), (bond, 1), (angle, 1)):
        del calls[:]
        monkeypatch.delenv("DM_NO_FUSED_MLP_FWD", raising=False)
        fused = run(HipOps(), torch.float32, False)
        assert len(calls) == n_mlps, "the fused primitive was not used"
        monkeypatch.setenv("DM_NO_FUSED_MLP_FWD", "1")
        chain = run(HipOps(), torch.float32, False)
        assert len(calls) == n_mlps, "DM_NO_FUSED_MLP_FWD=1 still used it"
        monkeypatch.delenv("DM_NO_FUSED_MLP_FWD")
        ref = run(CpuRefOps(), torch.float64, True)
        assert len(fused) == len(chain) == len(ref)
        for i, (f, c, r) in enumerate(zip(fused, chain, ref)):
            _bound(f, r, c, f"{run.__name__} out[{i}]")
