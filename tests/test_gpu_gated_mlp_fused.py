"""GPU tests of the whole gated MLP in one kernel (k_gated_mlp_64, entry
points dm_gated_mlp3_f32 / dm_gated_mlp4_f32): tile tails, guard regions,
every accepted form, the refusals, and the conv paths and the engine with
and without DM_NO_FUSED_MLP_FULL=1.

The reference everywhere is the kernel pair it replaces on the same inputs,
dm_edge_mlp3/4_f32 followed by dm_gated_mlp_tail_fwd_f32, and the check is
bitwise identity of z, c, g and out: both fma chains keep the pair's k order
(the first layer only swaps the operands of its MFMAs), so not a bit may
differ."""
import copy
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_atom_block import NAMES, _Case, _run  # noqa: E402
from test_gpu_mlp_tail_bwd import (D, E_SMALL, N_BONDS, N_NODES,  # noqa: E402
                                   _bound, _graphs, _mlp)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs HIP GPU")

GUARD = 256                 # floats on either side of z / c / g / out
SENTINEL = -12345.5
# Grid cap: 512 blocks of 4 waves, one 32-row tile per wave per iteration.
# 129*32+5 rows: 130 tiles in 33 blocks, ragged last tile, one tile per wave.
# 2049*32+5 rows: 2050 tiles > 2048 waves, so the first two waves take a
# second tile and the rest do not; the last tile is ragged.
E_MULTI_BLOCK = 129 * 32 + 5
E_MULTI_TILE = 2049 * 32 + 5
E_CASES = [1, 31, 32, 33, 63, 64, 65, E_MULTI_BLOCK, E_MULTI_TILE]
# (rows of the node tables, index pattern)
TABLES = [(1, "equal"), (37, "random"), (4099, "random"), (4099, "equal")]
# (keep, out, w, base)
FORMS = [(False, True, True, True), (False, True, True, False),
         (False, True, False, True), (False, True, False, False),
         (True, True, True, True), (True, True, True, False),
         (True, True, False, True), (True, False, False, False)]


def _fptr(t, off=0):
    return ctypes.cast(t.data_ptr() + 4 * off, ctypes.POINTER(ctypes.c_float))


def _iptr(t):
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_int32))


class _Data:
    """Inputs of E_MULTI_TILE rows over node tables of n rows; every case
    uses a prefix.  The pair's results are computed once per (ngather, E)
    and never modified."""

    def __init__(self, n, kind):
        dev = torch.device("cuda:0")
        gen = torch.Generator(device="cpu").manual_seed(4321 + n)
        E = E_MULTI_TILE
        self.dev, self.n = dev, n
        self.row = torch.randn(E, D, generator=gen).to(dev)
        self.wt = (torch.randn(D, 2 * D, generator=gen) / 8).to(dev)
        self.bias = torch.randn(2 * D, generator=gen).to(dev)
        self.tabs = [torch.randn(n, 2 * D, generator=gen).to(dev)
                     for _ in range(3)]
        self.idx = []
        for k in range(3):
            if kind == "equal":
                i = torch.full((E,), (n - 1) if k != 1 else n // 2)
            else:
                i = torch.randint(0, n, (E,), generator=gen)
                i[k] = n - 1                     # row N-1 within E = 31
                i[E - 1 - k] = n - 1
            self.idx.append(i.to(torch.int32).to(dev))
        self.w2 = (torch.randn(2, D, D, generator=gen) / 8).to(dev)
        self.b2 = torch.randn(2, 1, D, generator=gen).to(dev)
        self.w = torch.randn(E, D, generator=gen).to(dev)
        self.base = torch.randn(E, D, generator=gen).to(dev)
        self._pair = {}

    def pair(self, ng, E):
        """{"z", "c", "g", ("out", w, base)} of the two-kernel path."""
        if (ng, E) in self._pair:
            return self._pair[ng, E]
        from distmlip_amd.ops import _stream, hip_lib
        lib = hip_lib()
        z = torch.empty(E, 2 * D, device=self.dev)
        h = torch.empty(E, 2 * D, device=self.dev)
        t, i = self.tabs, self.idx
        if ng == 2:
            rc = lib.dm_edge_mlp3_f32(
                _fptr(self.row), _fptr(self.wt), _fptr(self.bias), _fptr(t[0]),
                _fptr(t[1]), _iptr(i[0]), _iptr(i[1]), _fptr(z), _fptr(h), E,
                D, 2 * D, _stream())
        else:
            rc = lib.dm_edge_mlp4_f32(
                _fptr(self.row), _fptr(self.wt), _fptr(self.bias), _fptr(t[0]),
                _fptr(t[1]), _fptr(t[2]), _iptr(i[0]), _iptr(i[1]),
                _iptr(i[2]), _fptr(z), _fptr(h), E, D, 2 * D, _stream())
        assert rc == 0
        res = {"z": z}
        for has_w in (True, False):
            for has_base in (True, False):
                c, g, out = (torch.empty(E, D, device=self.dev)
                             for _ in range(3))
                rc = lib.dm_gated_mlp_tail_fwd_f32(
                    _fptr(h), _fptr(self.w2), _fptr(self.w2, D * D),
                    _fptr(self.b2), _fptr(self.b2, D),
                    _fptr(self.w) if has_w else None,
                    _fptr(self.base) if has_base else None, _fptr(c),
                    _fptr(g), _fptr(out), E, D, _stream())
                assert rc == 0
                res["c"], res["g"] = c, g
                res["out", has_w, has_base] = out
        torch.cuda.synchronize()
        self._pair[ng, E] = res
        return res


_DATA = {}


def _data(n=4099, kind="random"):
    if (n, kind) not in _DATA:
        _DATA[n, kind] = _Data(n, kind)
    return _DATA[n, kind]


def _launch(d, ng, E, form, din=D, dim=D, expect_rc0=True, drop=()):
    """Run the kernel through the C entry point into guarded buffers on the
    first E rows.  Returns {"z", "c", "g", "out"} (None where the form does
    not take it) and asserts guards, full coverage of what the form takes
    and that nothing else was written.  drop names pointers passed as NULL
    although the form has them ("z", "c", "g", "out", "i0", "i1", "i2")."""
    from distmlip_amd.ops import _stream, hip_lib
    lib = hip_lib()
    keep, has_out, has_w, has_base = form
    sizes = {"z": E * 2 * D, "c": E * D, "g": E * D, "out": E * D}
    bufs = {k: torch.full((2 * GUARD + n,), SENTINEL, device=d.dev)
            for k, n in sizes.items()}
    views = {k: bufs[k][GUARD:GUARD + n] for k, n in sizes.items()}
    taken = {"z": keep, "c": keep, "g": keep, "out": has_out}
    ptr = {k: (_fptr(views[k]) if taken[k] and k not in drop else None)
           for k in sizes}
    ip = [None if f"i{k}" in drop else _iptr(d.idx[k]) for k in range(3)]
    t = d.tabs
    tail = (_fptr(d.w2), _fptr(d.w2, D * D), _fptr(d.b2), _fptr(d.b2, D),
            _fptr(d.w) if has_w else None,
            _fptr(d.base) if has_base else None,
            ptr["z"], ptr["c"], ptr["g"], ptr["out"], E, din, dim, _stream())
    if ng == 2:
        rc = lib.dm_gated_mlp3_f32(
            _fptr(d.row), _fptr(d.wt), _fptr(d.bias), _fptr(t[0]), _fptr(t[1]),
            ip[0], ip[1], *tail)
    else:
        rc = lib.dm_gated_mlp4_f32(
            _fptr(d.row), _fptr(d.wt), _fptr(d.bias), _fptr(t[0]), _fptr(t[1]),
            _fptr(t[2]), ip[0], ip[1], ip[2], *tail)
    torch.cuda.synchronize()
    if not expect_rc0:
        assert rc != 0
        for k, b in bufs.items():
            assert bool((b == SENTINEL).all()), f"a refused call wrote {k}"
        return None
    assert rc == 0, lib.dm_hip_last_error()
    for k, b in bufs.items():
        n = sizes[k]
        assert bool((b[:GUARD] == SENTINEL).all()), f"{k}: front guard"
        assert bool((b[GUARD + n:] == SENTINEL).all()), \
            f"{k}: rear guard written (E={E})"
        if taken[k]:
            assert not bool((views[k] == SENTINEL).any()), \
                f"{k}: rows left unwritten (E={E})"
        else:
            assert bool((b == SENTINEL).all()), \
                f"{k} written in a form that does not take it"
    return {"z": views["z"].view(E, 2 * D) if keep else None,
            "c": views["c"].view(E, D) if keep else None,
            "g": views["g"].view(E, D) if keep else None,
            "out": views["out"].view(E, D) if has_out else None}


def _first_diff(a, b):
    bad = (a != b).nonzero()
    return f"{int(bad.shape[0])} differ, first at {bad[0].tolist()}: " \
           f"{a[tuple(bad[0])].item()!r} vs {b[tuple(bad[0])].item()!r}"


def _check_forms(d, ng, E):
    ref = d.pair(ng, E)
    outs = {}
    for form in FORMS:
        keep, has_out, has_w, has_base = form
        got = _launch(d, ng, E, form)
        tag = f"ng={ng} E={E} n={d.n} form={form}"
        if keep:
            for k in ("z", "c", "g"):
                assert torch.equal(got[k], ref[k]), \
                    f"{k} {tag}: {_first_diff(got[k], ref[k])}"
        if has_out:
            want = ref["out", has_w, has_base]
            assert torch.equal(got["out"], want), \
                f"out {tag}: {_first_diff(got['out'], want)}"
            # keep and no-keep forms of one (w, base) give one out
            prev = outs.setdefault((has_w, has_base), got["out"])
            assert torch.equal(prev, got["out"])
        again = _launch(d, ng, E, form)
        for k, v in got.items():
            if v is not None:
                assert torch.equal(v, again[k]), f"{k} {tag}: second launch"


@requires_gpu
@pytest.mark.parametrize("E", E_CASES)
@pytest.mark.parametrize("ng", [2, 3])
def test_tiles_tails_guards(ng, E):
    """Every accepted form at one row count: guards, coverage, bitwise
    identity with the kernel pair, between forms and between launches."""
    _check_forms(_data(), ng, E)


@requires_gpu
@pytest.mark.parametrize("n,kind", TABLES)
@pytest.mark.parametrize("ng", [2, 3])
def test_tables_and_indices(ng, n, kind):
    """Node tables of 1, 37 and 4099 rows, random and all-equal indices,
    row N-1 included."""
    d = _data(n, kind)
    assert all(int(i.max()) == n - 1 for i in d.idx[::2])
    _check_forms(d, ng, E_MULTI_BLOCK)


KEEP_FULL, NO_KEEP = (True, True, True, True), (False, True, True, True)


@requires_gpu
@pytest.mark.parametrize("ng", [2, 3])
@pytest.mark.parametrize("form", [KEEP_FULL, NO_KEEP])
@pytest.mark.parametrize("din,dim", [(32, 64), (128, 64), (64, 32), (64, 65),
                                     (64, 128)])
def test_other_widths_refused(ng, form, din, dim):
    _launch(_data(), ng, 70, form, din=din, dim=dim, expect_rc0=False)


@requires_gpu
@pytest.mark.parametrize("ng", [2, 3])
@pytest.mark.parametrize("form,drop", [
    (KEEP_FULL, ("c",)), (KEEP_FULL, ("g",)),        # exactly one of c / g
    (KEEP_FULL, ("c", "g")),                         # z without c|g
    (KEEP_FULL, ("z",)),                             # c|g without z
    (NO_KEEP, ("out",)),                             # no-keep without out
    (KEEP_FULL, ("i0",)), (NO_KEEP, ("i1",))])       # NULL index
def test_bad_forms_refused(ng, form, drop):
    _launch(_data(), ng, 70, form, expect_rc0=False, drop=drop)


@requires_gpu
def test_null_third_index_refused():
    _launch(_data(), 3, 70, NO_KEEP, expect_rc0=False, drop=("i2",))


@requires_gpu
def test_no_rows_no_launch():
    from distmlip_amd.ops import _stream, hip_lib
    d = _data()
    out = torch.full((64,), SENTINEL, device=d.dev)
    rc = hip_lib().dm_gated_mlp3_f32(
        _fptr(d.row), _fptr(d.wt), _fptr(d.bias), _fptr(d.tabs[0]),
        _fptr(d.tabs[1]), _iptr(d.idx[0]), _iptr(d.idx[1]), _fptr(d.w2),
        _fptr(d.w2, D * D), _fptr(d.b2), _fptr(d.b2, D), None, None, None,
        None, None, _fptr(out), 0, D, D, _stream())
    torch.cuda.synchronize()
    assert rc == 0 and bool((out == SENTINEL).all())


@requires_gpu
def test_act_forms_refuse_recording():
    """The no-grad forms do not silently drop a gradient."""
    from distmlip_amd.ops import HipOps
    pd, _ = _graphs(torch.device("cuda:0"))
    d = _data()
    a = d.row[:E_SMALL].clone().requires_grad_(True)
    t = d.tabs[0][:N_BONDS].contiguous()
    with pytest.raises(AssertionError):
        HipOps().gated_mlp4_act(a, d.wt, d.bias, t, t, t, pd, d.w2, d.b2)


# --------------------------------------------------------------------------
# conv paths with and without the switch
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graphs():
    return _graphs(torch.device("cuda:0"))


@pytest.fixture(scope="module")
def case(graphs):
    return _Case(graphs[0].src.device)


def _spy(monkeypatch):
    """Count raw_gated_mlp launches as (keep, want_out)."""
    import distmlip_amd.ops as ops_mod
    launches = []
    real = ops_mod.raw_gated_mlp

    def spy(*a, **k):
        launches.append((a[9], a[10] if len(a) > 10
                         else k.get("want_out", True)))
        return real(*a, **k)
    monkeypatch.setattr(ops_mod, "raw_gated_mlp", spy)
    return launches


def _both(monkeypatch, fn, launches, expect):
    """fn() with the one-kernel MLP and with DM_NO_FUSED_MLP_FULL=1; asserts
    the launches and returns both results."""
    for name in ("DM_NO_FUSED_MLP_FULL", "DM_NO_FUSED_MLP_FWD",
                 "DM_NO_FUSED_MLP"):
        monkeypatch.delenv(name, raising=False)
    del launches[:]
    new = fn()
    assert launches == expect, launches
    monkeypatch.setenv("DM_NO_FUSED_MLP_FULL", "1")
    old = fn()
    assert launches == expect, "DM_NO_FUSED_MLP_FULL=1 still ran the kernel"
    monkeypatch.delenv("DM_NO_FUSED_MLP_FULL")
    return new, old


def _flat(x):
    out = []
    for t in x:
        if isinstance(t, (tuple, list)):
            out += _flat(t)
        else:
            out.append(t)
    return out


def _assert_same(new, old, what):
    new, old = _flat(new), _flat(old)
    assert len(new) == len(old)
    for i, (a, b) in enumerate(zip(new, old)):
        assert (a is None) == (b is None), f"{what}[{i}]"
        if a is not None:
            assert torch.equal(a, b), f"{what}[{i}]: {_first_diff(a, b)}"


def _atom_inputs(case):
    from distmlip_amd.chgnet import _packed_weights
    c = case
    wbb, wab = c.bexp @ c.Wbb.t(), c.bexp @ c.Wab.t()
    pe, pn = (_packed_weights(m) for m in c.mlps[0])
    return c.v, c.e, wbb, wab, pe, pn


@requires_gpu
@pytest.mark.parametrize("saves_only", [False, True])
def test_atom_fwd_switch(monkeypatch, graphs, case, saves_only):
    """conv.atom_fwd in keep form: both MLPs as one kernel each, the node
    MLP without out in a recomputation; every output and save bitwise equal
    to the pair's, and within the project's bound of fp64 plain torch."""
    from distmlip_amd import conv
    from distmlip_amd.chgnet import _packed_weights
    from distmlip_amd.ops import HipOps
    from oracle.chgnet_ref import CpuRefOps
    pd, pr = graphs
    v, e, wbb, wab, pe, pn = _atom_inputs(case)
    launches = _spy(monkeypatch)

    def fn():
        return conv.atom_fwd(HipOps(), pd, v, e, wbb, wab, pe, pn, D,
                             saves_only=saves_only)
    new, old = _both(monkeypatch, fn, launches,
                     [(True, True), (True, not saves_only)])
    _assert_same(new, old, f"atom_fwd saves_only={saves_only}")
    p64 = [_packed_weights(copy.deepcopy(m).double()) for m in case.mlps[0]]
    ref = conv.atom_fwd(CpuRefOps(), pr, v.double(), e.double(), wbb.double(),
                        wab.double(), p64[0], p64[1], D,
                        saves_only=saves_only)
    for i, (a, b, r) in enumerate(zip(_flat(new), _flat(old), _flat(ref))):
        if a is not None:
            _bound(a, r, b, f"atom_fwd saves_only={saves_only} [{i}]")


@requires_gpu
def test_lean_atom_unchanged(monkeypatch, graphs, case):
    """conv._lean_atom keeps the kernel pair (tests/test_gpu_atom_block.py
    counts its first-layer calls): no launch of the one-kernel MLP, same
    bits with and without the switch."""
    from distmlip_amd import conv
    from distmlip_amd.ops import HipOps
    pd, _ = graphs
    v, e, wbb, wab, pe, pn = _atom_inputs(case)
    launches = _spy(monkeypatch)

    def fn():
        with torch.no_grad():
            return conv._lean_atom(HipOps(), pd, v, e, wbb, wab, pe, pn, D)
    new, old = _both(monkeypatch, fn, launches, [])
    _assert_same(new, old, "_lean_atom")


@requires_gpu
def test_lean_line_graph_switch(monkeypatch, graphs):
    """conv._lean_bond / _lean_angle: the three-gather no-keep form."""
    from distmlip_amd import conv
    from distmlip_amd.chgnet import _packed_weights
    from distmlip_amd.ops import HipOps
    from oracle.chgnet_ref import CpuRefOps
    pd, pr = graphs
    pd.line_src_csr = (pd.line_src_perm, pd.line_src_row_ptr)
    pr.line_src_csr = None
    dev = pd.src.device
    gen = torch.Generator(device="cpu").manual_seed(61)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen).to(dev)

    n, a, v, w3 = rnd(N_BONDS, D), rnd(E_SMALL, D), rnd(N_NODES, D), \
        rnd(N_BONDS, D)
    pb, pa = (_packed_weights(_mlp(4, dev, s)) for s in (3, 4))
    launches = _spy(monkeypatch)

    def fn():
        with torch.no_grad():
            return (conv._lean_bond(HipOps(), pd, n, a, v, w3, pb, D),
                    conv._lean_angle(HipOps(), pd, n, a, v, pa, D))
    new, old = _both(monkeypatch, fn, launches, [(False, True)] * 2)
    _assert_same(new, old, "_lean_bond/_lean_angle")
    pb64, pa64 = (_packed_weights(_mlp(4, dev, s).double()) for s in (3, 4))
    n64, a64, v64, w64 = (t.double() for t in (n, a, v, w3))
    with torch.no_grad():
        ref = (conv._lean_bond(CpuRefOps(), pr, n64, a64, v64, w64, pb64, D),
               conv._lean_angle(CpuRefOps(), pr, n64, a64, v64, pa64, D))
    for name, g, o, r in zip(("_lean_bond", "_lean_angle"), new, old, ref):
        _bound(g, r, o, name)


@requires_gpu
@pytest.mark.parametrize("masked", [False, True])
def test_atom_block_switch(monkeypatch, graphs, case, masked):
    """_AtomBlockFn, two blocks chained: outputs and all gradients bitwise
    equal with and without the switch (its backward recomputes in keep
    form: one keep and one out-less launch per block), and within the
    project's bound of fp64 plain torch on the CPU backend."""
    from distmlip_amd.ops import HipOps
    from oracle.chgnet_ref import CpuRefOps
    pd, pr = graphs
    launches = _spy(monkeypatch)

    def fn():
        return _run(case, pd, HipOps(), torch.float32, "block", 2, masked,
                    True)
    new, old = _both(monkeypatch, fn, launches,
                     [(True, True), (True, False)] * 2)
    _assert_same(new, old, f"_AtomBlockFn masked={masked}")
    ref = _run(case, pr, CpuRefOps(), torch.float64, "plain", 2, masked, True)
    for name, g, o, r in zip(NAMES, new, old, ref):
        _bound(g, r, o, f"_AtomBlockFn {name} masked={masked}")


# --------------------------------------------------------------------------
# engine level
# --------------------------------------------------------------------------
@requires_gpu
@pytest.mark.parametrize("checkpoint", ["on", "off"])
def test_engine_switch(monkeypatch, checkpoint):
    """One SpmdEngine step on 320 atoms, checkpointed (self-recomputing atom
    blocks) and not (the whole-graph keep path with the bond graph): energy,
    forces and every other output equal with and without the switch."""
    from distmlip_amd.model import CHGNetCore
    from distmlip_amd.runtime import SpmdEngine
    from distmlip_amd.structures import diamond_si
    s = diamond_si((10, 2, 2), jitter=0.1, seed=3)
    core = CHGNetCore.seeded(seed=0).float()
    launches = _spy(monkeypatch)

    def run():
        eng = SpmdEngine(core, world=1, threads=2, device="cuda:0",
                         checkpoint=checkpoint)
        out = eng.step(s)
        return {k: v.detach().clone() for k, v in out.items()
                if torch.is_tensor(v)}

    monkeypatch.delenv("DM_NO_FUSED_MLP_FULL", raising=False)
    new = run()
    assert launches, "the one-kernel MLP was not used"
    n_new = len(launches)
    monkeypatch.setenv("DM_NO_FUSED_MLP_FULL", "1")
    old = run()
    assert len(launches) == n_new, "DM_NO_FUSED_MLP_FULL=1 still used it"
    assert set(new) == set(old) and "energy" in new and "forces_owned" in new
    for k in new:
        assert torch.equal(new[k], old[k]), f"{k}: {_first_diff(new[k], old[k])}"
