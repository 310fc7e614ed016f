"""GPU tests of the factored message weights (ops.RadialW): the "factored w"
state of k_gated_mlp_tail_fwd, k_gated_mlp_64 and k_gated_mlp_tail_bwd
(entry points dm_gated_mlp_tail_fwd_fw_f32, dm_gated_mlp3_fw_f32,
dm_gated_mlp_tail_bwd_fw_f32), which take bexp [E,9], W [64,9] and a mask [E]
and use w = mask * (bexp @ W.t()) without a dense [E,64] array, and the
atom-conv block that hands them over (conv._AtomBlockFn).

Accuracy bound everywhere (the _bound rule of tests/test_gpu_mlp_tail_bwd.py):
max |err| against an fp64 torch composition at most 2x that of the dense path
on the same inputs: w = bexp @ W.t() in fp32 torch, the existing kernel, and
dw @ W for dbexp.  Both are fp32 fma chains of the same lengths in different
orders."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_mlp_tail_bwd import D, _bound, _f64_tail  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs HIP GPU")

N_RBF = 9
N_TABLE = 40                       # node table of the indexed forms
E_MANY = 4 * 32 * 3 + 5            # 13 tiles: more than one block's 4 waves
E_CASES = [1, 31, 32, 167, E_MANY]  # 167 = 5 tiles + 7
GUARD = 64
SENTINEL = -12345.5


class _Data:
    """One set of inputs of E_MANY rows; every case uses a prefix.  Nothing
    is modified after construction."""

    def __init__(self):
        dev = torch.device("cuda:0")
        gen = torch.Generator(device="cpu").manual_seed(909)
        E = E_MANY

        def rnd(*shape):
            return torch.randn(*shape, generator=gen)

        bexp = rnd(E, N_RBF)
        bexp[torch.rand(E, generator=gen) < 0.15] = 0.0    # all-zero rows
        bexp[0] = 0.0
        self.bexp = bexp.to(dev)
        self.W = (rnd(D, N_RBF) / 3).to(dev)
        mask = (torch.rand(E, generator=gen) < 0.7).float()
        mask[:2] = torch.tensor([1.0, 0.0])[:2]
        self.mask = mask.to(dev)
        self.h = rnd(E, 2 * D).to(dev)
        self.w2 = (rnd(2, D, D) / 8).to(dev)
        self.b2 = (rnd(2, 1, D) / 4).to(dev)
        self.base = rnd(E, D).to(dev)
        self.cg = rnd(2, E, D).to(dev)
        self.z = rnd(E, 2 * D).to(dev)
        self.go = rnd(E, D).to(dev)
        self.go_tab = rnd(N_TABLE, D).to(dev)
        self.go_idx = torch.sort(torch.randint(
            0, N_TABLE, (E,), generator=gen)).values.to(torch.int32).to(dev)
        self.dbexp_in = rnd(E, N_RBF).to(dev)
        # whole-MLP operands
        self.erow = rnd(E, D).to(dev)
        self.wt = (rnd(D, 2 * D) / 8).to(dev)
        self.bias = (rnd(2 * D) / 4).to(dev)
        self.zs = rnd(N_TABLE, 2 * D).to(dev)
        self.zd = rnd(N_TABLE, 2 * D).to(dev)
        self.src = torch.randint(0, N_TABLE, (E,), generator=gen).to(
            torch.int32).to(dev)
        self.dst = self.go_idx
        self.dev = dev

    def w32(self, E, masked):
        """the dense path's weight: fp32 torch"""
        w = self.bexp[:E] @ self.W.t()
        return w * self.mask[:E, None] if masked else w

    def w64(self, E, masked):
        w = self.bexp[:E].double() @ self.W.double().t()
        return w * self.mask[:E, None].double() if masked else w

    def rw(self, E, masked, acc=None):
        from distmlip_amd.ops import RadialW
        return RadialW(self.bexp[:E], self.W,
                       self.mask[:E] if masked else None, acc)


@pytest.fixture(scope="module")
def data():
    return _Data()


def _out64(cg64, w64, base):
    x = torch.nn.functional.silu(cg64[0]) * torch.sigmoid(cg64[1]) * w64
    return x + base.double() if base is not None else x


# --------------------------------------------------------------------------
# forward tail (mlp_tail_act's no-keep form, and the keep form)
# --------------------------------------------------------------------------
@requires_gpu
@pytest.mark.parametrize("E", E_CASES)
@pytest.mark.parametrize("keep,has_base,masked", [
    (False, True, True), (False, False, False), (True, True, False),
    (True, False, True)])
def test_tail_fwd(data, keep, has_base, masked, E):
    from distmlip_amd.ops import raw_mlp_tail_fwd
    d = data
    h, base = d.h[:E], d.base[:E] if has_base else None
    out_d, cg_d = raw_mlp_tail_fwd(h, d.w2, d.b2, d.w32(E, masked), base, keep)
    out_f, cg_f = raw_mlp_tail_fwd(h, d.w2, d.b2, d.rw(E, masked), base, keep)
    if keep:
        assert torch.equal(cg_f, cg_d), "c|g differ from the dense entry's"
    else:
        assert cg_f is None
    cg64 = torch.baddbmm(d.b2.double(),
                         h.double().view(-1, 2, D).transpose(0, 1),
                         d.w2.double())
    _bound(out_f, _out64(cg64, d.w64(E, masked), base), out_d,
           f"tail fwd out keep={keep} base={has_base} mask={masked} E={E}")
    out_2, _ = raw_mlp_tail_fwd(h, d.w2, d.b2, d.rw(E, masked), base, keep)
    assert torch.equal(out_2, out_f)


# --------------------------------------------------------------------------
# the one-kernel MLP (r_gated_mlp3's keep-with-out form, and no-keep)
# --------------------------------------------------------------------------
def _gated_mlp(d, E, w, base, keep):
    from distmlip_amd.ops import raw_gated_mlp
    return raw_gated_mlp(d.erow[:E], d.wt, d.bias, (d.zs, d.zd),
                         (d.src[:E], d.dst[:E]), d.w2, d.b2, w, base, keep)


@requires_gpu
@pytest.mark.parametrize("E", E_CASES)
@pytest.mark.parametrize("keep,has_base,masked", [
    (True, True, True), (True, False, False), (False, True, False),
    (False, False, True)])
def test_gated_mlp3(data, keep, has_base, masked, E):
    d = data
    base = d.erow[:E] if has_base else None
    z_d, cg_d, out_d = _gated_mlp(d, E, d.w32(E, masked), base, keep)
    z_f, cg_f, out_f = _gated_mlp(d, E, d.rw(E, masked), base, keep)
    if keep:
        assert torch.equal(z_f, z_d), "z differs from the dense entry's"
        assert torch.equal(cg_f, cg_d), "c|g differ from the dense entry's"
    else:
        assert z_f is None and cg_f is None
    z64 = (d.erow[:E].double() @ d.wt.double() + d.bias.double()
           + d.zs.double()[d.src[:E].long()] + d.zd.double()[d.dst[:E].long()])
    h64 = torch.nn.functional.silu(z64)
    cg64 = torch.baddbmm(d.b2.double(), h64.view(-1, 2, D).transpose(0, 1),
                         d.w2.double())
    _bound(out_f, _out64(cg64, d.w64(E, masked), base), out_d,
           f"gated_mlp3 out keep={keep} base={has_base} mask={masked} E={E}")


# --------------------------------------------------------------------------
# reverse tail, plain and indexed, through the C entry into guarded buffers
# --------------------------------------------------------------------------
def _fptr(t, off=0):
    return ctypes.cast(t.data_ptr() + 4 * off, ctypes.POINTER(ctypes.c_float))


def _bwd_fw(d, E, indexed, masked, din_mode, dim=D, n_rbf=N_RBF,
            expect_rc0=True):
    """dm_gated_mlp_tail_bwd_fw_f32 on the first E rows.  din_mode: None,
    "separate" or "alias".  Returns (dz, dbexp); asserts the guards."""
    from distmlip_amd.ops import _stream, hip_lib
    lib = hip_lib()
    cg = d.cg[:, :E].contiguous()
    go = d.go_tab if indexed else d.go[:E]
    idx = ctypes.cast(d.go_idx.data_ptr(), ctypes.POINTER(ctypes.c_int32)) \
        if indexed else None
    zbuf = torch.full((2 * GUARD + E * 2 * D,), SENTINEL, device=d.dev)
    bbuf = torch.full((2 * GUARD + E * N_RBF,), SENTINEL, device=d.dev)
    dz = zbuf[GUARD:GUARD + E * 2 * D].view(E, 2 * D)
    dbexp = bbuf[GUARD:GUARD + E * N_RBF].view(E, N_RBF)
    din = None
    if din_mode == "separate":
        din = d.dbexp_in[:E].clone()
    elif din_mode == "alias":
        dbexp.copy_(d.dbexp_in[:E])
        din = dbexp
    bexp = d.bexp[:E].contiguous()
    rc = lib.dm_gated_mlp_tail_bwd_fw_f32(
        _fptr(go), idx, _fptr(cg), _fptr(cg, E * D), _fptr(bexp), _fptr(d.W),
        _fptr(d.mask) if masked else None, _fptr(d.z), _fptr(d.w2),
        _fptr(d.w2, D * D), _fptr(dz),
        _fptr(din) if din is not None else None, _fptr(dbexp), E, dim, n_rbf,
        _stream())
    torch.cuda.synchronize()
    if not expect_rc0:
        assert rc != 0
        assert bool((zbuf == SENTINEL).all())
        assert bool((bbuf == SENTINEL).all())
        return None, None
    assert rc == 0, lib.dm_hip_last_error()
    for name, buf, n in (("dz", zbuf, E * 2 * D), ("dbexp", bbuf, E * N_RBF)):
        assert bool((buf[:GUARD] == SENTINEL).all()), f"{name}: front guard"
        assert bool((buf[GUARD + n:] == SENTINEL).all()), \
            f"{name}: rear guard written (E={E})"
        assert not bool((buf[GUARD:GUARD + n] == SENTINEL).any()), \
            f"{name}: rows left unwritten (E={E})"
    if din_mode == "separate":
        assert torch.equal(din, d.dbexp_in[:E]), "dbexp_in was modified"
    return dz, dbexp


@requires_gpu
@pytest.mark.parametrize("E", E_CASES)
@pytest.mark.parametrize("indexed,masked,din_mode", [
    (False, True, None), (False, False, "separate"), (True, True, "alias"),
    (True, False, None), (False, True, "alias")])
def test_tail_bwd(data, indexed, masked, din_mode, E):
    from distmlip_amd.ops import raw_mlp_tail_bwd
    d = data
    cg = d.cg[:, :E].contiguous()
    go = d.go_tab if indexed else d.go[:E]
    idx = d.go_idx[:E] if indexed else None
    z = d.z[:E]
    # dense path: GEMM w, the existing kernel, dw @ W
    dz_d, dw_d = raw_mlp_tail_bwd(go, cg, d.w32(E, masked), z, d.w2, idx)
    if masked:
        dw_d = dw_d * d.mask[:E, None]
    dbexp_d = dw_d @ d.W
    go_rows = d.go_tab[d.go_idx[:E].long()] if indexed else go
    dz64, dw64 = _f64_tail(go_rows, cg[0], cg[1], d.w64(E, masked), z, d.w2)
    if masked:
        dw64 = dw64 * d.mask[:E, None].double()
    dbexp64 = dw64 @ d.W.double()
    if din_mode is not None:
        dbexp_d = dbexp_d + d.dbexp_in[:E]
        dbexp64 = dbexp64 + d.dbexp_in[:E].double()
    dz_f, dbexp_f = _bwd_fw(d, E, indexed, masked, din_mode)
    what = f"idx={indexed} mask={masked} din={din_mode} E={E}"
    _bound(dz_f, dz64, dz_d, "tail bwd dz " + what)
    _bound(dbexp_f, dbexp64, dbexp_d, "tail bwd dbexp " + what)
    # every way of passing dbexp_in gives the same bits
    if din_mode is not None:
        other = "separate" if din_mode == "alias" else "alias"
        dz_o, dbexp_o = _bwd_fw(d, E, indexed, masked, other)
        assert torch.equal(dz_o, dz_f) and torch.equal(dbexp_o, dbexp_f)
    # and HipOps.r_mlp_tail_bwd is that entry
    from distmlip_amd.ops import HipOps
    acc = d.dbexp_in[:E].clone() if din_mode is not None else None
    dz_a, dbexp_a = HipOps().r_mlp_tail_bwd(go, cg, d.rw(E, masked, acc), z,
                                            d.w2, idx)
    assert torch.equal(dz_a, dz_f) and torch.equal(dbexp_a, dbexp_f)
    assert acc is None or dbexp_a.data_ptr() == acc.data_ptr()


# --------------------------------------------------------------------------
# one w in all three kernels, masks, refusals
# --------------------------------------------------------------------------
@requires_gpu
@pytest.mark.parametrize("masked", [False, True])
def test_same_w_in_all_three_kernels(data, masked):
    """With c = 32 and g = 40 in every element, sigmoid(c) = sigmoid(g) = 1
    exactly in fp32, so the combine factor silu(c) * sigmoid(g) is 32 and
    out = 32 * w, an exact scaling; in the reverse, dc = go * w with go = 1,
    carried to dz unchanged by an identity second layer and z = 40
    (silu'(z) = 1 exactly).  The effective w of the three kernels is then
    read off bit for bit."""
    from distmlip_amd.ops import raw_mlp_tail_bwd, raw_mlp_tail_fwd
    d, E = data, E_MANY
    dev = d.dev
    w2_zero = torch.zeros(2, D, D, device=dev)
    b2 = torch.empty(2, 1, D, device=dev)
    b2[0], b2[1] = 32.0, 40.0
    rw = d.rw(E, masked)
    w_fwd = raw_mlp_tail_fwd(d.h, w2_zero, b2, rw, None, False)[0] / 32
    from distmlip_amd.ops import raw_gated_mlp
    w_mlp = raw_gated_mlp(d.erow, d.wt, d.bias, (d.zs, d.zd), (d.src, d.dst),
                          w2_zero, b2, rw, None, True)[2] / 32
    cg = torch.empty(2, E, D, device=dev)
    cg[0], cg[1] = 32.0, 40.0
    eye = torch.eye(D, device=dev).repeat(2, 1, 1).contiguous()
    dz, _ = raw_mlp_tail_bwd(torch.ones(E, D, device=dev), cg, rw,
                             torch.full((E, 2 * D), 40.0, device=dev), eye)
    w_bwd = dz[:, :D]
    assert torch.equal(w_fwd, w_mlp), "forward tail vs one-kernel MLP"
    assert torch.equal(w_fwd, w_bwd), "forward tail vs reverse tail"
    # and it is the weight: fp32 rounding of a 9-term sum away from fp64
    w64 = d.w64(E, masked)
    tol = 16 * torch.finfo(torch.float32).eps * (
        d.bexp.double().abs() @ d.W.double().abs().t())
    assert bool(((w_fwd.double() - w64).abs() <= tol).all())


@requires_gpu
@pytest.mark.parametrize("E", [31, 167])
def test_mask(data, E):
    from distmlip_amd.ops import RadialW, raw_mlp_tail_fwd
    d = data
    off = d.mask[:E] == 0
    assert bool(off.any()) and not bool(off.all())
    base = d.base[:E]
    out = raw_mlp_tail_fwd(d.h[:E], d.w2, d.b2, d.rw(E, True), base, False)[0]
    assert torch.equal(out[off], base[off]), "mask = 0 rows: out != base"
    _, _, out3 = _gated_mlp(d, E, d.rw(E, True), base, True)
    assert torch.equal(out3[off], base[off])
    for indexed in (False, True):
        _, dbexp = _bwd_fw(d, E, indexed, True, "separate")
        assert torch.equal(dbexp[off], d.dbexp_in[:E][off]), \
            "mask = 0 rows: dbexp != dbexp_in"
    # no mask is a mask of ones, bit for bit
    ones = RadialW(d.bexp[:E], d.W, torch.ones(E, 1, device=d.dev))
    a = raw_mlp_tail_fwd(d.h[:E], d.w2, d.b2, ones, base, False)[0]
    b = raw_mlp_tail_fwd(d.h[:E], d.w2, d.b2, d.rw(E, False), base, False)[0]
    assert torch.equal(a, b)
    assert torch.equal(_gated_mlp(d, E, ones, base, True)[2],
                       _gated_mlp(d, E, d.rw(E, False), base, True)[2])
    from distmlip_amd.ops import raw_mlp_tail_bwd
    cg = d.cg[:, :E].contiguous()
    ra = raw_mlp_tail_bwd(d.go[:E], cg, ones, d.z[:E], d.w2)
    rb = raw_mlp_tail_bwd(d.go[:E], cg, d.rw(E, False), d.z[:E], d.w2)
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])


@requires_gpu
@pytest.mark.parametrize("dim,n_rbf", [(64, 8), (64, 10), (32, 9), (128, 9)])
def test_other_sizes_refused(data, dim, n_rbf):
    """d != 64 or n_rbf != 9: an error, and nothing is launched."""
    from distmlip_amd.ops import _stream, hip_lib
    d, E = data, 70
    lib = hip_lib()
    _bwd_fw(d, E, False, True, None, dim=dim, n_rbf=n_rbf, expect_rc0=False)
    out = torch.full((E, D), SENTINEL, device=d.dev)
    cg = torch.full((2, E, D), SENTINEL, device=d.dev)
    z = torch.full((E, 2 * D), SENTINEL, device=d.dev)
    tail = (_fptr(d.w2), _fptr(d.w2, D * D), _fptr(d.b2), _fptr(d.b2, D),
            _fptr(d.bexp), _fptr(d.W), _fptr(d.mask), _fptr(d.base))
    rc = lib.dm_gated_mlp_tail_fwd_fw_f32(
        _fptr(d.h), *tail, _fptr(cg), _fptr(cg, E * D), _fptr(out), E, dim,
        n_rbf, _stream())
    assert rc != 0
    ip = ctypes.POINTER(ctypes.c_int32)
    rc = lib.dm_gated_mlp3_fw_f32(
        _fptr(d.erow), _fptr(d.wt), _fptr(d.bias), _fptr(d.zs), _fptr(d.zd),
        ctypes.cast(d.src.data_ptr(), ip), ctypes.cast(d.dst.data_ptr(), ip),
        *tail, _fptr(z), _fptr(cg), _fptr(cg, E * D), _fptr(out), E, 64, dim,
        n_rbf, _stream())
    assert rc != 0
    torch.cuda.synchronize()
    for t in (out, cg, z):
        assert bool((t == SENTINEL).all())


# --------------------------------------------------------------------------
# block level
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def block():
    from test_gpu_atom_block import _Case
    from test_gpu_mlp_tail_bwd import _graphs
    graphs = _graphs(torch.device("cuda:0"))
    return graphs, _Case(graphs[0].src.device)


def _count_block_w(monkeypatch):
    from distmlip_amd import conv
    calls = []
    real = conv._block_w
    monkeypatch.setattr(conv, "_block_w",
                        lambda *a: (calls.append(1), real(*a))[1])
    return calls


@requires_gpu
@pytest.mark.parametrize("masked", [False, True])
def test_block_builds_no_dense_weight(monkeypatch, block, masked):
    """Default switches: no _block_w call in forward or backward, the e2 of
    the save-nothing forward is the recomputation's bit for bit (the same w
    in both), and outputs and gradients hold the bound against fp64 relative
    to the dense path."""
    from distmlip_amd import conv
    from distmlip_amd.ops import HipOps
    from oracle.chgnet_ref import CpuRefOps
    from test_gpu_atom_block import NAMES, _run
    (pd, pr), case = block
    monkeypatch.delenv("DM_NO_FACTORED_W", raising=False)
    calls = _count_block_w(monkeypatch)
    e2s = []
    real_fwd = conv._mlp_fwd

    def mlp_fwd(ops, pd_, v, ebox, packs, w, base, d, want_out=True):
        r = real_fwd(ops, pd_, v, ebox, packs, w, base, d, want_out)
        if want_out:
            e2s.append(r[2])
        return r

    monkeypatch.setattr(conv, "_mlp_fwd", mlp_fwd)
    got = _run(case, pd, HipOps(), torch.float32, "block", 2, masked, True)
    assert not calls, f"{len(calls)} dense weights built"
    # blocks recompute in reverse order: the last recomputed e2 is block 1's
    # input e of block 2, the first is the block output
    assert len(e2s) == 2 and torch.equal(e2s[0], got[1]), \
        "recomputed e2 differs from the outer forward's"
    monkeypatch.setenv("DM_NO_FACTORED_W", "1")
    dense = _run(case, pd, HipOps(), torch.float32, "block", 2, masked, True)
    assert len(calls) == 8, f"{len(calls)} _block_w calls for 2 blocks"
    ref = _run(case, pr, CpuRefOps(), torch.float64, "plain", 2, masked, True)
    for name, g, o, r in zip(NAMES, got, dense, ref):
        _bound(g, r, o, f"{name} factored block mask={masked}")


@requires_gpu
def test_block_switch_restores_dense(monkeypatch, block):
    """DM_NO_FACTORED_W=1 is the path of a backend without the capability,
    bit for bit, and hands no RadialW to any primitive."""
    from distmlip_amd.ops import HipOps, RadialW
    from test_gpu_atom_block import _run
    (pd, _), case = block

    class Dense(HipOps):
        factored_w = False

    seen = []
    real = HipOps.r_mlp_tail_bwd

    def tail(self, go, cg, w, z, w2, go_idx=None):
        seen.append(isinstance(w, RadialW))
        return real(self, go, cg, w, z, w2, go_idx)

    monkeypatch.setattr(HipOps, "r_mlp_tail_bwd", tail)
    monkeypatch.setenv("DM_NO_FACTORED_W", "1")
    a = _run(case, pd, HipOps(), torch.float32, "block", 2, True, True)
    assert seen and not any(seen)
    monkeypatch.delenv("DM_NO_FACTORED_W")
    b = _run(case, pd, Dense(), torch.float32, "block", 2, True, True)
    assert not any(seen)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    del seen[:]
    _run(case, pd, HipOps(), torch.float32, "block", 2, True, True)
    assert seen and all(seen)
