"""CPU tests of the edge <-> bond row exchange of checkpointed steps
(conv.edge_to_bond / conv.bond_to_edge) on the torch-index fallback a backend
without r_move_rows takes: fp64, against the two out-of-place index_copy
lines of runtime.step, every value and every gradient EQUAL (the pair only
removes sums with exact zeros), e's storage reused, one backward call per
Function; and SpmdEngine(checkpoint="on") with and without
DM_NO_ROW_EXCHANGE=1."""
import pytest
import torch

from distmlip_amd import conv

D = 8
E = 40


class _PD:
    pass


def _pd(B, M, seed):
    gen = torch.Generator().manual_seed(seed)
    pd = _PD()
    pd.n_bonds = B
    pd.map_de = torch.randperm(E, generator=gen)[:M].contiguous()
    pd.map_ude = torch.arange(M)
    return pd


def _inputs(B, seed):
    gen = torch.Generator().manual_seed(seed)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float64)

    return dict(e=rnd(E, D), n=rnd(B, D), w_n=rnd(B, D), w_e=rnd(E, D),
                go_e=rnd(E, D), go_n=rnd(B, D), go_n2=rnd(B, D))


def _layer(x, pd, pair, n_grad, use_nc):
    """One layer's exchange around a stand-in bond conv, from leaves
    (e0, n0): e = 2*e0 (a block's output), n_c, n2 = f(n_c), e' and the
    later uses of e', n_c, n2.  Returns values and leaf gradients."""
    e0 = x["e"].clone().requires_grad_(True)
    n0 = x["n"].clone().requires_grad_(n_grad)
    e = e0 * 2
    n_prev = n0 * 3 if n_grad else n0
    if pair:
        e_id = e.data_ptr()
        e, n_c = conv.edge_to_bond(e, n_prev, pd, None)
        assert e.data_ptr() == e_id
    else:
        n_c = n_prev.index_copy(0, pd.map_ude, e[pd.map_de])
    w_n = x["w_n"].clone().requires_grad_(True)
    n2 = (n_c * w_n).sin() if use_nc else (n_prev * w_n).sin()
    n2.retain_grad()
    if pair:
        e_new = conv.bond_to_edge(e, n2, pd, None)
        assert e_new.data_ptr() == e_id, "bond_to_edge must write in place"
    else:
        e_new = e.index_copy(0, pd.map_de, n2[pd.map_ude])
    loss = ((e_new * x["w_e"]).cos() * x["go_e"]).sum() \
        + (n2 * x["go_n2"]).sum()
    if use_nc:
        loss = loss + (n_c * x["go_n"]).sum()
    loss.backward()
    return dict(n_c=n_c.detach(), e_new=e_new.detach(), de=e0.grad,
                dn=n0.grad, dn2=n2.grad, dw=w_n.grad)


CASES = [  # B, M
    (12, 12),       # every bond row owned
    (17, 12),       # ghost bond rows keep n_prev and pass their gradient
    (12, 0),        # nothing mapped
]


@pytest.mark.parametrize("B,M", CASES)
@pytest.mark.parametrize("n_grad", [True, False])
@pytest.mark.parametrize("use_nc", [True, False])
def test_pair_equals_index_copy_lines(B, M, n_grad, use_nc):
    """use_nc=False: n_c feeds nothing, its gradient arrives as None.
    n_grad=False: the initial n of a step, built on an empty buffer."""
    pd = _pd(B, M, seed=B * 100 + M)
    x = _inputs(B, seed=7)
    ref = _layer(x, pd, False, n_grad, use_nc)
    got = _layer(x, pd, True, n_grad, use_nc)
    for k in ref:
        if ref[k] is None:
            assert got[k] is None or not got[k].any(), k
            continue
        assert got[k] is not None, k
        assert torch.equal(got[k], ref[k]), \
            f"{k}: max diff {(got[k] - ref[k]).abs().max().item():.3e}"


def test_one_backward_call_each_and_inputs_untouched(monkeypatch):
    """Each Function's backward runs once per step (the single-consumer
    chain), and writes to no incoming gradient."""
    calls = {"e2b": 0, "b2e": 0}
    seen = []
    real_a, real_b = conv._EdgeToBondFn.backward, conv._BondToEdgeFn.backward

    def wrap_a(ctx, G_e, G_nc):
        calls["e2b"] += 1
        keep = [(g, g.clone()) for g in (G_e, G_nc) if g is not None]
        out = real_a(ctx, G_e, G_nc)
        seen.extend(keep)
        return out

    def wrap_b(ctx, go):
        calls["b2e"] += 1
        keep = [(go, go.clone())]
        out = real_b(ctx, go)
        seen.extend(keep)
        return out

    monkeypatch.setattr(conv._EdgeToBondFn, "backward", staticmethod(wrap_a))
    monkeypatch.setattr(conv._BondToEdgeFn, "backward", staticmethod(wrap_b))
    pd = _pd(17, 12, seed=5)
    _layer(_inputs(17, seed=9), pd, True, True, True)
    assert calls == {"e2b": 1, "b2e": 1}
    assert seen
    for g, before in seen:
        assert torch.equal(g, before), "an incoming gradient was written to"


def _engine(monkeypatch, env):
    from distmlip_amd.model import CHGNetCore
    from distmlip_amd.runtime import SpmdEngine
    from distmlip_amd.structures import diamond_si
    from oracle.chgnet_ref import CpuRefOps
    for k in ("DM_NO_ROW_EXCHANGE", "DM_NO_FINAL_KEEP"):
        monkeypatch.delenv(k, raising=False)
    for k in env:
        monkeypatch.setenv(k, "1")
    s = diamond_si((4, 2, 2), jitter=0.1, seed=3)
    core = CHGNetCore.seeded(seed=0).double()
    eng = SpmdEngine(core, world=1, threads=2, device="cpu", ops=CpuRefOps(),
                     checkpoint="on")
    return eng.step(s), len(core.bond_convs)


def test_engine_checkpointed_cpu(monkeypatch):
    """fp64 CpuRefOps engine, checkpoint="on": the pair (fallback path) is
    taken twice per bond layer plus once for the initial n, and energy and
    forces equal the torch lines'."""
    n_fwd = []
    real = conv._move_rows
    monkeypatch.setattr(
        conv, "_move_rows",
        lambda *a, **k: (n_fwd.append(torch.is_grad_enabled()), real(*a, **k))[1])
    got, n_bond = _engine(monkeypatch, ())
    assert len(n_fwd) > 0
    n_fwd.clear()
    ref, _ = _engine(monkeypatch, ("DM_NO_ROW_EXCHANGE",))
    assert not n_fwd, "DM_NO_ROW_EXCHANGE=1 still took the Function pair"
    assert torch.equal(got["energy"], ref["energy"])
    assert torch.equal(got["forces_owned"], ref["forces_owned"])
    fwd = []
    real_a, real_b = conv._EdgeToBondFn.forward, conv._BondToEdgeFn.forward
    monkeypatch.setattr(conv._EdgeToBondFn, "forward", staticmethod(
        lambda *a: (fwd.append("e2b"), real_a(*a))[1]))
    monkeypatch.setattr(conv._BondToEdgeFn, "forward", staticmethod(
        lambda *a: (fwd.append("b2e"), real_b(*a))[1]))
    _engine(monkeypatch, ())
    assert fwd.count("e2b") == n_bond + 1 and fwd.count("b2e") == n_bond, fwd
