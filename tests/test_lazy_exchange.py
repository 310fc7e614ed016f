"""CPU tests (fp64) of the lazy edge/bond row exchange: the reverses of
conv.edge_to_bond / conv.bond_to_edge that copy nothing and leave the
exchanged rows of the e gradient to the consuming block's r_edge_mlp_bwd
(conv.ExchangeHolder, conv.slot_map, mlp_path.lazy_exchange).

 * SpmdEngine(checkpoint="on") with CpuRefOps, which has no r_edge_mlp_bwd:
   the step materialises as before, with and without DM_NO_LAZY_EXCHANGE=1.
 * The wiring itself on a torch backend that has the raw first layer and a
   patch-taking r_edge_mlp_bwd: two _AtomBlockFn blocks around one boundary,
   lazy against copying, every output and gradient EQUAL, no copy of an
   [E,d] gradient, one patched call.
 * A second consumer of e, or a gradient that is not the tensor handed on,
   raises instead of leaking stale rows.
 * atom_bwd materialises where the kernel that takes the patch does not run.
"""
import pytest
import torch

from distmlip_amd import conv, mlp_path
from distmlip_amd.chgnet import _packed_weights
from distmlip_amd.model import GatedMLP
from oracle.chgnet_ref import CpuRefOps

D, N, E, B, M, N_RBF = 64, 19, 157, 40, 33, 9


class _PatchOps(CpuRefOps):
    """CpuRefOps plus the raw fused first layer and its reverse with the
    patch argument, in plain torch."""

    edge_mlp_bwd_patch = True

    def __init__(self):
        self.patched = []

    def r_edge_mlp3(self, erow, wt, bias, zs, zd, pd):
        z = erow @ wt + bias + zs[pd.src] + zd[pd.dst]
        return z, torch.nn.functional.silu(z)

    def r_edge_mlp_bwd(self, dz, wt, gbase=None, out=None, patch=None):
        if patch is not None:
            slot, rows = patch
            self.patched.append(int((slot >= 0).sum()))
            sel = slot >= 0
            gbase = torch.where(sel[:, None], rows[slot.clamp(min=0).long()],
                                gbase)
        res = dz @ wt.t() if gbase is None else gbase + dz @ wt.t()
        if out is not None:
            return out.copy_(res)
        return res


class _PD:
    pass


def _graph():
    gen = torch.Generator().manual_seed(5)
    pd = _PD()
    pd.n_atoms, pd.n_bonds = N, B
    pd.src = torch.randint(0, N, (E,), generator=gen)
    pd.dst = torch.sort(torch.randint(0, N, (E,), generator=gen)).values
    pd.map_de = torch.randperm(E, generator=gen)[:M].contiguous()
    pd.map_ude = torch.randperm(B, generator=gen)[:M].contiguous()
    return pd


def _mlp(seed):
    torch.manual_seed(seed)
    mlp = GatedMLP(3 * D, D, D).double()
    for p in mlp.parameters():
        p.requires_grad_(False)
    return mlp


class _Case:
    def __init__(self):
        gen = torch.Generator().manual_seed(8)

        def rnd(*shape):
            return torch.randn(*shape, generator=gen, dtype=torch.float64)

        self.pd = _graph()
        self.v, self.e, self.n = rnd(N, D), rnd(E, D), rnd(B, D)
        self.bexp = rnd(E, N_RBF)
        self.Wbb, self.Wab = rnd(D, N_RBF) / 3, rnd(D, N_RBF) / 3
        self.w_n = rnd(B, D)
        self.go_v, self.go_e, self.go_n = rnd(N, D), rnd(E, D), rnd(B, D)
        self.packs = [(_packed_weights(_mlp(1 + 2 * i)),
                       _packed_weights(_mlp(2 + 2 * i))) for i in range(2)]


@pytest.fixture(scope="module")
def case():
    return _Case()


@pytest.fixture
def clean_env(monkeypatch):
    for name in list(mlp_path.SWITCHES) + [mlp_path.NO_LAZY_EXCHANGE]:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def _chain(c, ops, lazy, tamper=None, use_nc=True):
    """block 0 -> edge_to_bond -> a stand-in bond conv -> bond_to_edge ->
    block 1, from leaves; returns the outputs and the leaf gradients."""
    pd = c.pd
    v, e0, n0, bexp = (t.clone().requires_grad_(True)
                       for t in (c.v, c.e, c.n, c.bexp))
    holder = conv.ExchangeHolder() if lazy else None
    pe, pn = c.packs[0]
    x_v, x_e = conv._AtomBlockFn.apply(v, e0 * 2, bexp, c.Wbb, c.Wab, None,
                                       pd, ops, pe, pn, D, holder)
    assert holder is None or holder.bound
    x_e, n_c = conv.edge_to_bond(x_e, n0 * 3, pd, ops, holder)
    extra = (x_e * c.go_e).sum() if tamper == "second_consumer" else 0
    n2 = ((n_c if use_nc else n0) * c.w_n).sin()
    x_e = conv.bond_to_edge(x_e, n2, pd, ops, holder)
    pe, pn = c.packs[1]
    y_v, y_e = conv._AtomBlockFn.apply(x_v, x_e, bexp, c.Wbb, c.Wab, None,
                                       pd, ops, pe, pn, D)
    loss = (y_v * c.go_v).sum() + (y_e * c.go_e).sum() \
        + (n2 * c.go_n).sum() + extra
    loss.backward()
    return dict(y_v=y_v.detach(), y_e=y_e.detach(), dv=v.grad, de=e0.grad,
                dn=n0.grad, dbexp=bexp.grad)


@pytest.mark.parametrize("use_nc", [True, False])
def test_lazy_chain_equals_copying_chain(clean_env, case, use_nc):
    """use_nc=False: n_c feeds nothing, so edge_to_bond's reverse gets no
    G_nc and has to zero the stale rows itself."""
    assert mlp_path.lazy_exchange(_PatchOps(), D)
    assert not mlp_path.lazy_exchange(CpuRefOps(), D)
    owned = []
    real_own = conv._own
    clean_env.setattr(conv, "_own",
                      lambda g: (owned.append(g.shape[0]), real_own(g))[1])
    ops_old, ops_new = _PatchOps(), _PatchOps()
    old = _chain(case, ops_old, lazy=False, use_nc=use_nc)
    assert owned.count(E) == (2 if use_nc else 1) and not ops_old.patched
    del owned[:]
    new = _chain(case, ops_new, lazy=True, use_nc=use_nc)
    for k in old:
        assert torch.equal(new[k], old[k]), k
    if use_nc:
        assert E not in owned, "a reverse of the exchange copied [E,d]"
        assert ops_new.patched == [M]
    else:
        assert owned.count(E) == 1 and not ops_new.patched


def test_unbound_holder_copies(clean_env, case):
    """A holder that no block took is not used by the exchange."""
    pd, ops = case.pd, _PatchOps()
    holder = conv.ExchangeHolder()
    e0 = case.e.clone().requires_grad_(True)
    n0 = case.n.clone().requires_grad_(True)
    e, n_c = conv.edge_to_bond(e0 * 2, n0 * 3, pd, ops, holder)
    e = conv.bond_to_edge(e, (n_c * case.w_n).sin(), pd, ops, holder)
    ((e * case.go_e).sum()).backward()
    assert not holder.pending and holder.patch is None
    ref_e0 = case.e.clone().requires_grad_(True)
    ref_n0 = case.n.clone().requires_grad_(True)
    e = ref_e0 * 2
    n_c = (ref_n0 * 3).index_copy(0, pd.map_ude, e[pd.map_de])
    e = e.index_copy(0, pd.map_de, (n_c * case.w_n).sin()[pd.map_ude])
    ((e * case.go_e).sum()).backward()
    assert torch.equal(e0.grad, ref_e0.grad)
    assert torch.equal(n0.grad, ref_n0.grad)


def test_second_consumer_of_e_raises(clean_env, case):
    with pytest.raises(RuntimeError, match="lazy edge/bond exchange"):
        _chain(case, _PatchOps(), lazy=True, tamper="second_consumer")
    # the copying reverses take the same graph
    _chain(case, _PatchOps(), lazy=False, tamper="second_consumer")


def test_holder_checks_identity():
    h = conv.ExchangeHolder()
    assert h.receive(torch.zeros(3, 2)) is None        # nothing was sent
    g, p = torch.randn(5, 2), torch.randn(2, 2)
    h.send(g, patch=p)
    assert h.pending and h.receive(g) is p and not h.pending
    h.send(g, patch=p)
    with pytest.raises(RuntimeError):
        h.receive(g.clone())                           # a copy of it
    assert not h.pending and h.patch is None
    h.send(g, patch=p)
    g.add_(1)                                          # written to since
    with pytest.raises(RuntimeError):
        h.receive(g)
    h.send(g)
    with pytest.raises(RuntimeError):
        h.receive(None)


def test_slot_map_is_cached_per_maps(case):
    pd = _graph()
    slot = conv.slot_map(pd, E)
    assert slot.dtype == torch.int32 and slot.shape == (E,)
    want = torch.full((E,), -1, dtype=torch.int32)
    want[pd.map_de] = pd.map_ude.to(torch.int32)
    assert torch.equal(slot, want) and int((slot >= 0).sum()) == M
    assert conv.slot_map(pd, E) is slot
    pd.map_de = pd.map_de.flip(0).contiguous()         # the maps are rebuilt
    slot2 = conv.slot_map(pd, E)
    assert slot2 is not slot and not torch.equal(slot2, slot)
    assert torch.equal(slot2[pd.map_de], pd.map_ude.to(torch.int32))


@pytest.mark.parametrize("how", ["no_go_v2", "no_kernel", "no_patch_arg"])
def test_atom_bwd_materialises(clean_env, case, how):
    """Where the node MLP's r_edge_mlp_bwd does not run (go_v2 None, the
    rocBLAS first-layer reverse, a backend without the patch argument),
    atom_bwd given a patch equals atom_bwd given the patched gradient, and
    the stale gradient is not written to."""
    c, pd = case, case.pd
    ops = CpuRefOps() if how == "no_patch_arg" else _PatchOps()
    if how == "no_kernel":
        clean_env.setenv("DM_NO_FUSED_MLP1_BWD", "1")
    pe, pn = c.packs[0]
    gen = torch.Generator().manual_seed(3)
    wbb = torch.randn(E, D, generator=gen, dtype=torch.float64)
    wab = torch.randn(E, D, generator=gen, dtype=torch.float64)
    G_nc = torch.randn(B, D, generator=gen, dtype=torch.float64)
    go_v = None if how == "no_go_v2" else c.go_v
    stale = c.go_e.clone()
    whole = c.go_e.clone().index_copy_(0, pd.map_de, G_nc[pd.map_ude])

    def run(go_e, patch):
        saved = conv.atom_fwd(ops, pd, c.v, c.e, wbb, wab, pe, pn, D)[2]
        return conv.atom_bwd(ops, pd, saved, pe, pn, D, wbb, wab, go_v, go_e,
                             patch=patch)

    want, got = run(whole, None), run(stale, G_nc)
    assert torch.equal(stale, c.go_e)
    assert not getattr(ops, "patched", None)
    for a, b in zip(got, want):
        assert (a is None and b is None) or torch.equal(a, b)


def _engine(monkeypatch, off):
    from distmlip_amd.model import CHGNetCore
    from distmlip_amd.runtime import SpmdEngine
    from distmlip_amd.structures import diamond_si
    monkeypatch.delenv(mlp_path.NO_LAZY_EXCHANGE, raising=False)
    if off:
        monkeypatch.setenv(mlp_path.NO_LAZY_EXCHANGE, "1")
    s = diamond_si((4, 2, 2), jitter=0.1, seed=3)
    core = CHGNetCore.seeded(seed=0).double()
    eng = SpmdEngine(core, world=1, threads=2, device="cpu", ops=CpuRefOps(),
                     checkpoint="on")
    return eng.step(s)


def test_engine_checkpointed_cpu(clean_env):
    """The fp64 reference backend has no patch-taking kernel: the step
    copies as before whatever the switch says, and nothing is left to a
    holder."""
    sent = []
    real = conv.ExchangeHolder.send
    clean_env.setattr(conv.ExchangeHolder, "send",
                      lambda self, *a, **k: (sent.append(1),
                                             real(self, *a, **k))[1])
    on, off = _engine(clean_env, False), _engine(clean_env, True)
    assert not sent
    assert torch.equal(on["energy"], off["energy"])
    assert torch.equal(on["forces_owned"], off["forces_owned"])
