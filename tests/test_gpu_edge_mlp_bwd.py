"""GPU tests of the first layer's reverse kernel (k_edge_mlp_bwd, entry point
dm_edge_mlp_bwd_f32: out = (gbase +) dz @ WT^T) and of the indexed form of
the reverse tail (dm_gated_mlp_tail_bwd_idx_f32): tile tails, guard regions,
accuracy against fp64 relative to the rocBLAS call each replaces, in-place
operation, bitwise repeatability, the shape guards, and the gradients of
_EdgeMlp3 / _EdgeMlp4 with the kernel and with DM_NO_FUSED_MLP1_BWD=1.

The accuracy bound everywhere: max |err| against fp64 at most 2x that of the
fp32 rocBLAS path on the same inputs (two equally long fp32 fma chains in
different orders), the bound tests/test_gpu_edge_mlp_mfma.py uses."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_mlp_tail_bwd import (D, E_CASES, E_MULTI_TILE,  # noqa: E402
                                   E_SMALL, GUARD, N_BONDS, N_NODES, SENTINEL,
                                   _bound, _fptr, _graphs, _leaves, _mlp)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs HIP GPU")

N_TABLE = 50                # rows of the indexed tail's go table


class _Data:
    """One set of inputs of E_MULTI_TILE rows; every case uses a prefix.
    References are computed once and never modified."""

    def __init__(self):
        dev = torch.device("cuda:0")
        gen = torch.Generator(device="cpu").manual_seed(9753)
        E = E_MULTI_TILE
        self.dev = dev
        self.dz = torch.randn(E, 2 * D, generator=gen).to(dev)
        self.gbase = torch.randn(E, D, generator=gen).to(dev)
        self.wt = (torch.randn(D, 2 * D, generator=gen) / 8).to(dev)
        mm64 = self.dz.double() @ self.wt.double().t()
        self.ref = {
            False: (mm64, self.dz @ self.wt.t()),
            True: (self.gbase.double() + mm64,
                   torch.addmm(self.gbase, self.dz, self.wt.t())),
        }
        # reverse-tail inputs
        self.cg = torch.randn(2, E, D, generator=gen).to(dev)
        self.w = torch.randn(E, D, generator=gen).to(dev)
        self.z = torch.randn(E, 2 * D, generator=gen).to(dev)
        self.w2 = (torch.randn(2, D, D, generator=gen) / 8).to(dev)
        self.go = torch.randn(E, D, generator=gen).to(dev)
        self.table = torch.randn(N_TABLE, D, generator=gen).to(dev)
        self.idx_rand = torch.randint(0, N_TABLE, (E,), generator=gen).to(
            torch.int32).to(dev)

    def idx_sorted(self, E):
        """A sorted index with repeats over the whole table, E entries."""
        return torch.sort(self.idx_rand[:E]).values.contiguous()


@pytest.fixture(scope="module")
def data():
    return _Data()


def _guarded(d, n):
    buf = torch.full((2 * GUARD + n,), SENTINEL, device=d.dev)
    return buf, buf[GUARD:GUARD + n]


def _check_guards(name, buf, n, E, written=True):
    assert bool((buf[:GUARD] == SENTINEL).all()), f"{name}: front guard"
    assert bool((buf[GUARD + n:] == SENTINEL).all()), \
        f"{name}: rear guard written (E={E})"
    if written:
        assert not bool((buf[GUARD:GUARD + n] == SENTINEL).any()), \
            f"{name}: elements left unwritten (E={E})"
    else:
        assert bool((buf == SENTINEL).all()), f"{name}: written"


def _launch(d, E, has_base, din=2 * D, dout=D, expect_rc0=True,
            in_place=False):
    """dm_edge_mlp_bwd_f32 into a guarded buffer on the first E rows; with
    in_place the buffer first holds gbase and is passed as both."""
    from distmlip_amd.ops import _stream, hip_lib
    lib = hip_lib()
    obuf, oview = _guarded(d, E * D)
    out = oview.view(E, D)
    gbase = d.gbase[:E] if has_base else None
    if in_place:
        out.copy_(d.gbase[:E])
        gbase = out
    rc = lib.dm_edge_mlp_bwd_f32(
        _fptr(d.dz[:E]), _fptr(d.wt), _fptr(gbase) if has_base else None,
        _fptr(out), E, din, dout, _stream())
    torch.cuda.synchronize()
    if not expect_rc0:
        assert rc != 0
        _check_guards("out", obuf, E * D, E, written=False)
        return None
    assert rc == 0, lib.dm_hip_last_error()
    _check_guards("out", obuf, E * D, E)
    return out


@requires_gpu
@pytest.mark.parametrize("E", E_CASES)
@pytest.mark.parametrize("has_base", [True, False])
def test_tiles_tails_guards(data, has_base, E):
    d = data
    ref64, ref32 = (t[:E] for t in d.ref[has_base])
    out = _launch(d, E, has_base)
    _bound(out, ref64, ref32, f"edge_mlp_bwd gbase={has_base} E={E}")
    assert torch.equal(_launch(d, E, has_base), out), "second launch differs"
    if has_base:
        assert torch.equal(_launch(d, E, True, in_place=True), out), \
            "out is gbase differs from out of place"


@requires_gpu
@pytest.mark.parametrize("din,dout", [(64, 64), (127, 64), (256, 64),
                                      (128, 32), (128, 65)])
def test_other_shapes_refused(data, din, dout):
    _launch(data, 70, True, din=din, dout=dout, expect_rc0=False)


@requires_gpu
def test_raw_wrapper(data):
    """raw_edge_mlp_bwd: the entry point's bits, fresh and in place."""
    from distmlip_amd.ops import HipOps, raw_edge_mlp_bwd
    d, E = data, 1000
    want = _launch(d, E, True)
    assert torch.equal(raw_edge_mlp_bwd(d.dz[:E], d.wt, d.gbase[:E]), want)
    own = d.gbase[:E].clone()
    got = HipOps().r_edge_mlp_bwd(d.dz[:E], d.wt, own, out=own)
    assert got is own and torch.equal(own, want)
    assert torch.equal(raw_edge_mlp_bwd(d.dz[:E], d.wt),
                       _launch(d, E, False))


# --------------------------------------------------------------------------
# indexed reverse tail
# --------------------------------------------------------------------------
def _tail(d, E, has_w, go, idx):
    """The plain (idx None, go [E,64]) or the indexed entry point into
    guarded dz / dw; the index array has exactly E entries."""
    from distmlip_amd.ops import _stream, hip_lib
    lib = hip_lib()
    cg = d.cg[:, :E].contiguous()
    w = d.w[:E] if has_w else None
    zbuf, zview = _guarded(d, E * 2 * D)
    wbuf, wview = _guarded(d, E * D)
    dz, dw = zview.view(E, 2 * D), wview.view(E, D)
    args = (_fptr(cg), _fptr(cg, E * D), _fptr(w) if has_w else None,
            _fptr(d.z[:E]), _fptr(d.w2), _fptr(d.w2, D * D), _fptr(dz),
            _fptr(dw) if has_w else None, E, D, _stream())
    if idx is None:
        rc = lib.dm_gated_mlp_tail_bwd_f32(_fptr(go), *args)
    else:
        # an allocation of exactly E entries, so nothing valid lies behind
        # idx[E-1].  The caching allocator rounds it up inside a larger
        # segment, so a read past it would neither fault nor show here; what
        # rules it out is the kernel, which loads idx[row] only under the
        # row < E predicate of its A phase
        idx_own = torch.empty(E, dtype=torch.int32, device=d.dev)
        idx_own.copy_(idx[:E])
        rc = lib.dm_gated_mlp_tail_bwd_idx_f32(
            _fptr(go), ctypes.cast(idx_own.data_ptr(),
                                   ctypes.POINTER(ctypes.c_int32)), *args)
    torch.cuda.synchronize()
    assert rc == 0, lib.dm_hip_last_error()
    _check_guards("dz", zbuf, E * 2 * D, E)
    _check_guards("dw", wbuf, E * D, E, written=has_w)
    return dz, (dw if has_w else None)


@requires_gpu
@pytest.mark.parametrize("E", E_CASES)
@pytest.mark.parametrize("has_w", [True, False])
def test_indexed_tail(data, has_w, E):
    d = data
    # identity index over go itself
    dz0, dw0 = _tail(d, E, has_w, d.go[:E], None)
    ident = torch.arange(E, dtype=torch.int32, device=d.dev)
    dz1, dw1 = _tail(d, E, has_w, d.go[:E], ident)
    assert torch.equal(dz1, dz0)
    # sorted index with repeats over a small table
    idx = d.idx_sorted(E)
    gathered = d.table[idx.long()].contiguous()
    dz2, dw2 = _tail(d, E, has_w, gathered, None)
    dz3, dw3 = _tail(d, E, has_w, d.table, idx)
    assert torch.equal(dz3, dz2)
    if has_w:
        assert torch.equal(dw1, dw0) and torch.equal(dw3, dw2)


@requires_gpu
def test_indexed_tail_wrapper_and_guards(data):
    from distmlip_amd.ops import HipOps, _stream, hip_lib
    d, E = data, 1000
    cg = d.cg[:, :E].contiguous()
    idx = d.idx_sorted(E)
    gathered = d.table[idx.long()].contiguous()
    a = HipOps().r_mlp_tail_bwd(gathered, cg, d.w[:E], d.z[:E], d.w2)
    b = HipOps().r_mlp_tail_bwd(d.table, cg, d.w[:E], d.z[:E], d.w2,
                                go_idx=idx)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # d != 64 and a missing index are refused and write nothing
    lib = hip_lib()
    zbuf, zview = _guarded(d, E * 2 * D)
    for dim, idx in ((32, idx), (64, None)):
        rc = lib.dm_gated_mlp_tail_bwd_idx_f32(
            _fptr(d.table),
            ctypes.cast(idx.data_ptr(), ctypes.POINTER(ctypes.c_int32))
            if idx is not None else None,
            _fptr(cg), _fptr(cg, E * D), None, _fptr(d.z[:E]), _fptr(d.w2),
            _fptr(d.w2, D * D), _fptr(zview), None, E, dim, _stream())
        torch.cuda.synchronize()
        assert rc != 0
        _check_guards("dz", zbuf, E * 2 * D, E, written=False)


# --------------------------------------------------------------------------
# through autograd: _EdgeMlp3 / _EdgeMlp4 input gradients
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graphs():
    return _graphs(torch.device("cuda:0"))


@requires_gpu
@pytest.mark.parametrize("kind", [3, 4])
def test_autograd(monkeypatch, graphs, kind):
    """Gradients of one gated_mlp_split call (first layer _EdgeMlp3/4): the
    kernel, DM_NO_FUSED_MLP1_BWD=1 (rocBLAS), and fp64 plain torch."""
    import copy

    import distmlip_amd.ops as ops_mod
    from distmlip_amd.chgnet import gated_mlp_split3, gated_mlp_split4
    from distmlip_amd.ops import HipOps
    from oracle.chgnet_ref import CpuRefOps
    pd, pr = graphs
    dev = pd.src.device
    gen = torch.Generator(device="cpu").manual_seed(19 + kind)
    mlp = _mlp(kind, dev, seed=23 + kind)
    mlp64 = copy.deepcopy(mlp).double()
    v = torch.randn(N_NODES, D, generator=gen).to(dev)
    e = torch.randn(E_SMALL, D, generator=gen).to(dev)
    n = torch.randn(N_BONDS, D, generator=gen).to(dev)
    w = torch.randn(E_SMALL, D, generator=gen).to(dev)
    go = torch.randn(E_SMALL, D, generator=gen).to(dev)

    def run(ops, m, p, dtype=torch.float32):
        if kind == 3:
            leaves = _leaves((e, v, w), dtype)
            out = gated_mlp_split3(m, leaves[1], leaves[0], p, ops, D,
                                   w=leaves[2], base=leaves[0])
        else:
            leaves = _leaves((e, n, v, w), dtype)
            out = gated_mlp_split4(m, leaves[1], leaves[0], leaves[2], p,
                                   ops, D, w=leaves[3])
        out.backward(go.to(dtype))
        return [t.grad for t in leaves]

    launches = []
    real = ops_mod.raw_edge_mlp_bwd
    monkeypatch.setattr(ops_mod, "raw_edge_mlp_bwd",
                        lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    monkeypatch.delenv("DM_NO_FUSED_MLP1_BWD", raising=False)
    fused = run(HipOps(), mlp, pd)
    assert len(launches) == 1, "dm_edge_mlp_bwd_f32 did not run"
    monkeypatch.setenv("DM_NO_FUSED_MLP1_BWD", "1")
    gemm = run(HipOps(), mlp, pd)
    assert len(launches) == 1, "DM_NO_FUSED_MLP1_BWD=1 still ran the kernel"
    ref = run(CpuRefOps(), mlp64, pr, torch.float64)
    for i, (f, c, r) in enumerate(zip(fused, gemm, ref)):
        _bound(f, r, c, f"split{kind} grad[{i}]")
