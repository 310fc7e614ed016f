"""GPU tests of the patched-gbase form of the first layer's reverse kernel
(k_edge_mlp_bwd<true, true>, entry point dm_edge_mlp_bwd_patch_f32,
HipOps.r_edge_mlp_bwd(..., patch=(slot, rows))): row r of gbase is read from
rows[slot[r]] where slot[r] >= 0.

The reference is the path it replaces, on the same device: a clone of gbase,
r_zero_rows and r_move_rows(add) over the patched rows, then the plain
r_edge_mlp_bwd.  The outputs must be EQUAL (torch.equal, == semantics: the
one difference the two paths can have is the sign of a zero, 0 + (-0) = +0).

And through SpmdEngine(checkpoint="on") on 320 atoms: the lazy exchange
(default) against DM_NO_LAZY_EXCHANGE=1, every returned array equal, no copy
of an [E,d] gradient in the exchange reverses, one patched launch per
edge/bond boundary."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_mlp_tail_bwd import D, GUARD, SENTINEL  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs HIP GPU")

E_MAX = 4096 + 5            # 33 blocks of 4 waves x 32 rows
E_CASES = [1003, 32, 31, E_MAX]
EXTRA = 7                   # rows of patch that no slot names


class _Data:
    """One set of inputs of E_MAX rows; every case uses a prefix."""

    def __init__(self):
        self.dev = dev = torch.device("cuda:0")
        gen = torch.Generator(device="cpu").manual_seed(20611)
        self.gen = gen
        self.dz = torch.randn(E_MAX, 2 * D, generator=gen).to(dev)
        self.gbase = torch.randn(E_MAX, D, generator=gen).to(dev)
        self.wt = (torch.randn(D, 2 * D, generator=gen) / 8).to(dev)
        self.patch = torch.randn(E_MAX + EXTRA, D, generator=gen)


@pytest.fixture(scope="module")
def data():
    return _Data()


def _rows(E, pattern):
    """The patched rows of a case, in ascending order."""
    if pattern == "none":
        return []
    if pattern == "all":
        return list(range(E))
    # mixed: rows 0 and E-1, two adjacent rows of one tile, and where there
    # are that many tiles, all of tile 1 and nothing of tile 2
    rows = {0, E - 1, min(5, E - 1), min(6, E - 1)}
    if E > 96:
        rows |= set(range(32, 64)) | {97, 98}
    return sorted(rows)


def _case(d, E, pattern):
    """(slot int32 [E], patch [M+EXTRA,64], rows int64 [M], src int64 [M]):
    row rows[i] is read from patch[src[i]], src in no order."""
    rows = _rows(E, pattern)
    M = len(rows)
    gen = torch.Generator(device="cpu").manual_seed(1000 * E + M)
    src = torch.randperm(M + EXTRA, generator=gen)[:M]
    patch = d.patch[:M + EXTRA].clone()
    if M >= 2:
        patch[src[0]] = 0.0              # exact zeros
        patch[src[1]] = -0.0             # negative zeros
    slot = torch.full((E,), -1, dtype=torch.int32)
    rows_t = torch.tensor(rows, dtype=torch.int64)
    slot[rows_t] = src.to(torch.int32)
    return (slot.to(d.dev), patch.to(d.dev), rows_t.to(d.dev),
            src.to(d.dev).contiguous())


def _reference(d, E, patch, rows, src):
    """Today's path: clone, zero the rows, add the bond-side rows, then the
    plain kernel."""
    from distmlip_amd.ops import HipOps
    ops = HipOps()
    g = d.gbase[:E].clone()
    if len(rows):
        ops.r_zero_rows(g, rows)
        ops.r_move_rows(patch, src, g, rows, add=True)
    return ops.r_edge_mlp_bwd(d.dz[:E], d.wt, g)


def _guarded(d, E):
    buf = torch.full((2 * GUARD + E * D,), SENTINEL, device=d.dev)
    return buf, buf[GUARD:GUARD + E * D].view(E, D)


def _check_guards(buf, E):
    n = E * D
    assert bool((buf[:GUARD] == SENTINEL).all()), "front guard written"
    assert bool((buf[GUARD + n:] == SENTINEL).all()), \
        f"rear guard written (E={E})"
    assert not bool((buf[GUARD:GUARD + n] == SENTINEL).any()), \
        f"elements left unwritten (E={E})"


@requires_gpu
@pytest.mark.parametrize("pattern", ["mixed", "none", "all"])
@pytest.mark.parametrize("E", E_CASES)
def test_patch_equals_clone_and_row_kernels(data, E, pattern):
    from distmlip_amd.ops import HipOps
    d, ops = data, HipOps()
    slot, patch, rows, src = _case(d, E, pattern)
    want = _reference(d, E, patch, rows, src)
    gbase0, patch0 = d.gbase[:E].clone(), patch.clone()
    # out a fresh buffer
    buf, out = _guarded(d, E)
    got = ops.r_edge_mlp_bwd(d.dz[:E], d.wt, d.gbase[:E], out=out,
                             patch=(slot, patch))
    torch.cuda.synchronize()
    assert got is out
    _check_guards(buf, E)
    assert torch.equal(got, want), \
        f"E={E} {pattern}: {(got != want).any(1).nonzero().flatten()[:8]}"
    if len(rows) >= 2:
        # the rows read from exact zeros and from negative zeros
        assert bool((got[rows[:2]] == want[rows[:2]]).all())
    assert torch.equal(d.gbase[:E], gbase0) and torch.equal(patch, patch0), \
        "an input was written to"
    # out is gbase
    buf, own = _guarded(d, E)
    own.copy_(d.gbase[:E])
    got = ops.r_edge_mlp_bwd(d.dz[:E], d.wt, own, out=own,
                             patch=(slot, patch))
    torch.cuda.synchronize()
    _check_guards(buf, E)
    assert got is own and torch.equal(own, want), f"in place E={E} {pattern}"
    # without out: a fresh result
    assert torch.equal(ops.r_edge_mlp_bwd(d.dz[:E], d.wt, d.gbase[:E],
                                          patch=(slot, patch)), want)


@requires_gpu
def test_wrapper_and_entry_refusals(data):
    from distmlip_amd.ops import _fp, _ip, _stream, hip_lib, raw_edge_mlp_bwd
    d, E = data, 70
    slot, patch, _, _ = _case(d, E, "mixed")
    with pytest.raises(AssertionError):       # patch rows must not be out
        full = torch.randn(E, D, device=d.dev)
        raw_edge_mlp_bwd(d.dz[:E], d.wt, d.gbase[:E], out=full,
                         patch=(slot, full))
    with pytest.raises(AssertionError):       # a patch needs a gbase
        raw_edge_mlp_bwd(d.dz[:E], d.wt, None, patch=(slot, patch))
    with pytest.raises(AssertionError):       # slot is int32 [E]
        raw_edge_mlp_bwd(d.dz[:E], d.wt, d.gbase[:E],
                         patch=(slot.long(), patch))
    lib = hip_lib()
    buf, out = _guarded(d, E)

    def entry(gbase, slot_, out_, din=2 * D, dout=D):
        return lib.dm_edge_mlp_bwd_patch_f32(
            _fp(d.dz[:E]), _fp(d.wt), gbase, slot_, _fp(patch), out_, E, din,
            dout, _stream())

    g = _fp(d.gbase[:E])
    assert entry(None, _ip(slot), _fp(out)) != 0
    assert entry(g, None, _fp(out)) != 0
    assert entry(g, _ip(slot), None) != 0
    assert entry(g, _ip(slot), _fp(patch)) != 0          # patch is out
    assert entry(g, _ip(slot), _fp(out), din=64) != 0
    assert entry(g, _ip(slot), _fp(out), dout=32) != 0
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()), "a refused call launched"


# --------------------------------------------------------------------------
# engine level
# --------------------------------------------------------------------------
@requires_gpu
def test_engine_lazy_exchange(monkeypatch):
    from distmlip_amd import conv
    from distmlip_amd.model import CHGNetCore
    from distmlip_amd.ops import HipOps
    from distmlip_amd.runtime import SpmdEngine
    from distmlip_amd.structures import diamond_si
    s = diamond_si((10, 2, 2), jitter=0.1, seed=3)
    core = CHGNetCore.seeded(seed=0).float()
    n_bond = len(core.bond_convs)
    log = []
    real_bwd = HipOps.r_edge_mlp_bwd

    def bwd(self, *a, patch=None, **k):
        log.append(("bwd", patch is not None, a[0].shape[0]))
        return real_bwd(self, *a, patch=patch, **k)

    real_own = conv._own
    monkeypatch.setattr(HipOps, "r_edge_mlp_bwd", bwd)
    monkeypatch.setattr(
        conv, "_own", lambda g: (log.append(("own", g.shape[0])),
                                 real_own(g))[1])

    def run(off):
        monkeypatch.delenv("DM_NO_LAZY_EXCHANGE", raising=False)
        if off:
            monkeypatch.setenv("DM_NO_LAZY_EXCHANGE", "1")
        del log[:]
        eng = SpmdEngine(core, world=1, threads=2, device="cuda:0",
                         checkpoint="on")
        out = eng.step(s)
        return {k: v.clone() for k, v in out.items()
                if torch.is_tensor(v)}, list(log)

    new, log_new = run(False)
    old, log_old = run(True)
    assert set(new) == set(old) and "forces_owned" in new
    for k in old:
        assert torch.equal(new[k], old[k]), k
    E = max(n for tag, *_, n in log_old if tag == "bwd")
    # the parent's reverses: two copies of the [E,d] gradient per boundary,
    # plus the initial edge_to_bond's
    assert [x for x in log_old if x == ("own", E)] == \
        [("own", E)] * (2 * n_bond + 1)
    assert not any(x[0] == "bwd" and x[1] for x in log_old)
    # lazy: only the initial edge_to_bond (no block before it) still copies
    assert [x for x in log_new if x == ("own", E)] == [("own", E)]
    assert sum(1 for x in log_new if x[0] == "bwd" and x[1]) == n_bond
    assert sum(1 for x in log_new if x[0] == "bwd") == \
        sum(1 for x in log_old if x[0] == "bwd")
