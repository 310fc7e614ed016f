"""GPU tests of the indexed row moves (csrc/rows.hip: dm_move_rows_f32,
dm_zero_rows_f32), of the Function pair built on them (conv.edge_to_bond /
conv.bond_to_edge) and of the final block that keeps its saves
(conv._AtomBlockKeepFn).  Everything here only MOVES fp32 values or adds one
pair of them, so every comparison is bit for bit (torch.equal): against the
torch index op each entry replaces, against the two index_copy lines of
runtime.step, against _AtomBlockFn, and through SpmdEngine(checkpoint="on")
against the DM_NO_ROW_EXCHANGE=1 / DM_NO_FINAL_KEEP=1 switches."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_mlp_tail_bwd import D, E_SMALL, N_NODES, _graphs, _mlp  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs HIP GPU")

R = 1000                    # rows of the tables
N_RBF = 9


def _fptr(t):
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_float)) \
        if t is not None else None


def _lptr(t):
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_int64)) \
        if t is not None else None


class _Data:
    """Tables of R rows for each width and one pair of unique index lists
    that includes row 0 and row R-1; prefixes serve every M."""

    def __init__(self):
        self.dev = torch.device("cuda:0")
        gen = torch.Generator(device="cpu").manual_seed(99)
        self.src = {d: torch.randn(R, d, generator=gen).to(self.dev)
                    for d in (64, 3, 1, 8)}
        self.dst = {d: torch.randn(R, d, generator=gen).to(self.dev)
                    for d in (64, 3, 1, 8)}

        def idx():
            p = torch.randperm(R, generator=gen)
            p = p[(p != 0) & (p != R - 1)]
            return torch.cat([torch.tensor([R - 1, 0]), p]).to(self.dev)

        self.si, self.di = idx(), idx()


@pytest.fixture(scope="module")
def data():
    return _Data()


def _move(src, si, dst, di, M, d, op):
    from distmlip_amd.ops import _stream, hip_lib
    rc = hip_lib().dm_move_rows_f32(_fptr(src), _lptr(si), _fptr(dst),
                                    _lptr(di), M, d, op, _stream())
    torch.cuda.synchronize()
    return rc


def _ref_move(src, si, dst, di, M, add):
    rows = src[si] if si is not None else src[:M]
    di = di if di is not None else torch.arange(M, device=dst.device)
    out = dst.clone()
    if add:
        return out.index_put_((di,), rows, accumulate=True)
    return out.index_copy_(0, di, rows)


@requires_gpu
@pytest.mark.parametrize("op", [0, 1])
@pytest.mark.parametrize("d,M", [(64, 0), (64, 1), (64, 3), (64, 257),
                                 (64, R), (3, 257), (1, 257), (8, 257)])
def test_move_rows_vs_torch(data, d, M, op):
    """float4 path at D = 64 (fixed width) and D = 8 (runtime width), scalar
    path at D = 3 and D = 1; M = R runs the unrolled loop and, at 257 rows,
    its tail; every other row of dst is untouched."""
    si, di = data.si[:M].contiguous(), data.di[:M].contiguous()
    dst = data.dst[d].clone()
    assert _move(data.src[d], si, dst, di, M, d, op) == 0
    assert torch.equal(dst, _ref_move(data.src[d], si, data.dst[d], di, M,
                                      op == 1))


@requires_gpu
@pytest.mark.parametrize("op", [0, 1])
@pytest.mark.parametrize("null", ["si", "di", "both"])
def test_move_rows_null_index(data, null, op):
    M, d = 257, 64
    si = None if null in ("si", "both") else data.si[:M].contiguous()
    di = None if null in ("di", "both") else data.di[:M].contiguous()
    dst = data.dst[d].clone()
    assert _move(data.src[d], si, dst, di, M, d, op) == 0
    assert torch.equal(dst, _ref_move(data.src[d], si, data.dst[d], di, M,
                                      op == 1))


@requires_gpu
def test_move_rows_unaligned_takes_scalar_path(data):
    """D = 64 from a source 4 bytes off a 16-byte boundary."""
    M, d = 257, 64
    buf = torch.empty(R * d + 1, device=data.dev)
    src = buf[1:].view(R, d)
    src.copy_(data.src[d])
    assert src.data_ptr() % 16 != 0
    si, di = data.si[:M].contiguous(), data.di[:M].contiguous()
    dst = data.dst[d].clone()
    assert _move(src, si, dst, di, M, d, 0) == 0
    assert torch.equal(dst, _ref_move(data.src[d], si, data.dst[d], di, M,
                                      False))


@requires_gpu
@pytest.mark.parametrize("d,M", [(64, 0), (64, 1), (64, 257), (64, R),
                                 (3, 257), (1, 3)])
@pytest.mark.parametrize("null", [False, True])
def test_zero_rows_vs_torch(data, d, M, null):
    from distmlip_amd.ops import _stream, hip_lib
    di = None if null else data.di[:M].contiguous()
    dst = data.dst[d].clone()
    rc = hip_lib().dm_zero_rows_f32(_fptr(dst), _lptr(di), M, d, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    ref = data.dst[d].clone()
    if null:
        ref[:M] = 0
    else:
        ref.index_fill_(0, di, 0)
    assert torch.equal(dst, ref)


@requires_gpu
def test_bad_arguments_launch_nothing(data):
    from distmlip_amd.ops import _stream, hip_lib
    lib = hip_lib()
    d, M = 64, 3
    si, di = data.si[:M].contiguous(), data.di[:M].contiguous()
    dst = data.dst[d].clone()
    assert _move(data.src[d], si, dst, di, M, d, 2) != 0        # op
    assert b"op" in lib.dm_hip_last_error()
    assert _move(data.src[d], si, dst, di, M, 0, 0) != 0        # D
    assert _move(None, si, dst, di, M, d, 0) != 0               # NULL src
    assert lib.dm_move_rows_f32(_fptr(data.src[d]), _lptr(si), None,
                                _lptr(di), M, d, 0, _stream()) != 0
    assert lib.dm_zero_rows_f32(None, _lptr(di), M, d, _stream()) != 0
    assert lib.dm_zero_rows_f32(_fptr(dst), _lptr(di), M, -1, _stream()) != 0
    torch.cuda.synchronize()
    assert torch.equal(dst, data.dst[d])
    # M <= 0 is a no-op, not an error
    assert _move(data.src[d], si, dst, di, -5, d, 0) == 0
    assert torch.equal(dst, data.dst[d])


@requires_gpu
def test_move_rows_offsets_past_2_31(data):
    """Destination rows whose element offsets need 64 bits: 2^25 + 8 rows of
    64 floats (8.6 GB, allocated and never filled), four rows moved to its
    last four rows, which start past element 2^31."""
    d, M = 64, 4
    rows = 2 ** 25 + 8
    big = torch.empty(rows, d, device=data.dev)
    di = torch.tensor([rows - 1, rows - 3, rows - 4, rows - 2],
                      device=data.dev)
    assert int(di.min()) * d >= 2 ** 31
    si = data.si[:M].contiguous()
    assert _move(data.src[d], si, big, di, M, d, 0) == 0
    assert torch.equal(big[di], data.src[d][si])
    big[di] = 1.0
    assert _move(data.src[d], si, big, di, M, d, 1) == 0
    assert torch.equal(big[di], 1.0 + data.src[d][si])
    from distmlip_amd.ops import raw_zero_rows
    raw_zero_rows(big, di)
    assert not big[rows - 4:].any()
    # and as the SOURCE of a gather
    big[rows - 4:] = data.src[d][:4]
    out = torch.empty(M, d, device=data.dev)
    assert _move(big, di, out, None, M, d, 0) == 0
    assert torch.equal(out, big[di])
    del big


class _PD:
    pass


@requires_gpu
@pytest.mark.parametrize("B,M", [(300, 300), (333, 300)])
@pytest.mark.parametrize("n_grad", [True, False])
def test_function_pair_vs_torch_lines(data, B, M, n_grad):
    """edge_to_bond / bond_to_edge with HipOps, fp32, against the two
    index_copy lines: values and the gradients on e, n_prev and n2 bit-equal,
    e's storage reused."""
    from distmlip_amd import conv
    from distmlip_amd.ops import HipOps
    ops = HipOps()
    pd = _PD()
    pd.n_bonds = B
    pd.map_de = data.di[:M].contiguous()
    pd.map_ude = torch.arange(M, device=data.dev)
    gen = torch.Generator(device="cpu").manual_seed(5)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen).to(data.dev)

    x_n, w_n, w_e = rnd(B, D), rnd(B, D), rnd(R, D)
    go_e, go_n, go_n2 = rnd(R, D), rnd(B, D), rnd(B, D)

    def run(pair):
        e0 = data.src[D].clone().requires_grad_(True)
        n0 = x_n.clone().requires_grad_(n_grad)
        e = e0 * 2
        n_prev = n0 * 3 if n_grad else n0
        if pair:
            e_id = e.data_ptr()
            e, n_c = conv.edge_to_bond(e, n_prev, pd, ops)
        else:
            n_c = n_prev.index_copy(0, pd.map_ude, e[pd.map_de])
        n2 = (n_c * w_n).sin()
        n2.retain_grad()
        if pair:
            e_new = conv.bond_to_edge(e, n2, pd, ops)
            assert e_new.data_ptr() == e_id
        else:
            e_new = e.index_copy(0, pd.map_de, n2[pd.map_ude])
        ((e_new * w_e).cos() * go_e).sum().add(
            (n2 * go_n2).sum()).add((n_c * go_n).sum()).backward()
        return dict(n_c=n_c.detach(), e_new=e_new.detach(), de=e0.grad,
                    dn=n0.grad, dn2=n2.grad)

    ref, got = run(False), run(True)
    for k in ref:
        if ref[k] is None:
            assert got[k] is None, k
        else:
            assert torch.equal(got[k], ref[k]), k


# --- the final block that keeps its saves -----------------------------------

@pytest.fixture(scope="module")
def graphs():
    return _graphs(torch.device("cuda:0"))


@requires_gpu
@pytest.mark.parametrize("with_go_e2", [True, False])
@pytest.mark.parametrize("masked", [False, True])
def test_keep_block_vs_atom_block(graphs, masked, with_go_e2):
    """_AtomBlockKeepFn against _AtomBlockFn on the small graph: outputs and
    all gradients bit-equal, and no forward kernel runs in its backward."""
    from distmlip_amd import conv
    from distmlip_amd.chgnet import _packed_weights
    from distmlip_amd.ops import HipOps
    pd, ops = graphs[0], HipOps()
    dev = pd.src.device
    gen = torch.Generator(device="cpu").manual_seed(404)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen).to(dev)

    xv, xe, xb = rnd(N_NODES, D), rnd(E_SMALL, D), rnd(E_SMALL, N_RBF)
    Wbb, Wab = rnd(D, N_RBF) / 3, rnd(D, N_RBF) / 3
    mask = (torch.rand(E_SMALL, 1, generator=gen) < 0.8).float().to(dev) \
        if masked else None
    go_v, go_e = rnd(N_NODES, D), rnd(E_SMALL, D)
    pe, pn = _packed_weights(_mlp(3, dev, 41)), _packed_weights(_mlp(3, dev, 42))

    def run(fn):
        v, e, bexp = (t.clone().requires_grad_(True) for t in (xv, xe, xb))
        v2, e2 = fn.apply(v, e, bexp, Wbb, Wab, mask, pd, ops, pe, pn, D)
        loss = (v2 * go_v).sum()
        if with_go_e2:
            loss = loss + (e2 * go_e).sum()
        real = conv.atom_fwd
        calls = []
        conv.atom_fwd = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        try:
            loss.backward()
        finally:
            conv.atom_fwd = real
        return (v2.detach(), e2.detach(), v.grad, e.grad, bexp.grad), \
            len(calls)

    ref, n_ref = run(conv._AtomBlockFn)
    got, n_got = run(conv._AtomBlockKeepFn)
    assert n_ref == 1 and n_got == 0
    for name, a, b in zip(("v2", "e2", "dv", "de", "dbexp"), got, ref):
        assert torch.equal(a, b), name


# --- engine level ------------------------------------------------------------

@requires_gpu
def test_engine_checkpointed_switches(monkeypatch):
    """SpmdEngine(checkpoint="on") on 320 atoms: the default against
    DM_NO_ROW_EXCHANGE=1 and against DM_NO_FINAL_KEEP=1, energy and forces
    bit-equal; r_move_rows runs in the forward twice per bond layer plus
    once for the initial n; with the keep block no atom_fwd runs after the
    forward's last one."""
    from distmlip_amd import conv
    from distmlip_amd.model import CHGNetCore
    from distmlip_amd.ops import HipOps
    from distmlip_amd.runtime import SpmdEngine
    from distmlip_amd.structures import diamond_si
    s = diamond_si((10, 2, 2), jitter=0.1, seed=3)
    core = CHGNetCore.seeded(seed=0).float()
    n_bond = len(core.bond_convs)
    n_atom = len(core.atom_convs)
    log = []
    real_move = HipOps.r_move_rows
    monkeypatch.setattr(
        HipOps, "r_move_rows",
        lambda self, *a, **k: (log.append("move"), real_move(self, *a, **k))[1])
    real_fwd = conv.atom_fwd
    monkeypatch.setattr(
        conv, "atom_fwd",
        lambda *a, **k: (log.append("atom_fwd"), real_fwd(*a, **k))[1])
    real_bwd = conv.atom_bwd
    monkeypatch.setattr(
        conv, "atom_bwd",
        lambda *a, **k: (log.append("atom_bwd"), real_bwd(*a, **k))[1])

    def run(env):
        for k in ("DM_NO_ROW_EXCHANGE", "DM_NO_FINAL_KEEP"):
            monkeypatch.delenv(k, raising=False)
        if env:
            monkeypatch.setenv(env, "1")
        del log[:]
        eng = SpmdEngine(core, world=1, threads=2, device="cuda:0",
                         checkpoint="on")
        out = eng.step(s)
        return out["energy"].clone(), out["forces_owned"].clone(), list(log)

    E_new, F_new, log_new = run(None)
    E_nox, F_nox, log_nox = run("DM_NO_ROW_EXCHANGE")
    E_nok, F_nok, log_nok = run("DM_NO_FINAL_KEEP")
    assert torch.equal(E_new, E_nox) and torch.equal(F_new, F_nox)
    assert torch.equal(E_new, E_nok) and torch.equal(F_new, F_nok)
    # forward moves come before the first reverse block
    first_bwd = log_new.index("atom_bwd")
    assert log_new[:first_bwd].count("move") == 2 * n_bond + 1
    assert "move" not in log_nox
    # keep block: its atom_fwd is in the forward, its atom_bwd follows with
    # no atom_fwd in between; each earlier block recomputes once
    assert log_new[:first_bwd].count("atom_fwd") == 1
    assert log_new[first_bwd:].count("atom_fwd") == n_atom - 1
    assert log_new.count("atom_bwd") == n_atom
    # without the keep block every atom_fwd is a recomputation, the first of
    # them right before the first atom_bwd
    i = log_nok.index("atom_bwd")
    assert log_nok[i - 1] == "atom_fwd" and log_nok.count("atom_fwd") == n_atom
