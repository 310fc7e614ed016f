"""CPU guard of conv.atom_fwd / conv.atom_bwd's fallback: with a backend that
lacks the optional raw primitives (CpuRefOps has neither r_edge_mlp3 nor
r_edge_mlp_bwd nor the indexed tail), 4-element and 5-element packs both
take the addmm / r_gather_add3 / r_gather_dst path, and that path's outputs
and gradients are those of autograd through the op-by-op block in fp64."""
import pytest
import torch

from distmlip_amd import conv
from distmlip_amd.chgnet import _packed_weights, gated_mlp_split3
from distmlip_amd.model import GatedMLP
from oracle.chgnet_ref import CpuRefOps

D, N, E = 64, 23, 301


class _PD:
    pass


def _graph():
    gen = torch.Generator().manual_seed(5)
    pd = _PD()
    pd.n_atoms = N
    pd.src = torch.randint(0, N, (E,), generator=gen)
    pd.dst = torch.sort(torch.randint(0, N, (E,), generator=gen)).values
    return pd


def _mlp(seed):
    torch.manual_seed(seed)
    mlp = GatedMLP(3 * D, D, D).double()
    for p in mlp.parameters():
        p.requires_grad_(False)
    return mlp


@pytest.mark.parametrize("with_go_e2", [True, False])
def test_atom_fwd_bwd_fallback(with_go_e2):
    ops = CpuRefOps()
    for name in ("r_edge_mlp3", "r_edge_mlp_bwd"):
        assert not hasattr(ops, name)
    pd = _graph()
    gen = torch.Generator().manual_seed(8)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float64)

    v, e, wbb, wab = rnd(N, D), rnd(E, D), rnd(E, D), rnd(E, D)
    go_v = rnd(N, D)
    go_e = rnd(E, D) if with_go_e2 else None
    m_e, m_n = _mlp(1), _mlp(2)

    # autograd through the op-by-op block
    lv = [t.clone().requires_grad_(True) for t in (v, e, wbb, wab)]
    e2 = gated_mlp_split3(m_e, lv[0], lv[1], pd, ops, D, w=lv[2], base=lv[1])
    msg = gated_mlp_split3(m_n, lv[0], e2, pd, ops, D, w=lv[3])
    v2 = ops.scatter_edges(msg, pd, base=lv[0])
    loss = (v2 * go_v).sum()
    if with_go_e2:
        loss = loss + (e2 * go_e).sum()
    loss.backward()
    want = (v2.detach(), e2.detach()) + tuple(t.grad for t in lv)

    outs = {}
    for n_pack in (4, 5):
        pe = _packed_weights(m_e)[:n_pack]
        pn = _packed_weights(m_n)[:n_pack]
        v2h, e2h, saved = conv.atom_fwd(ops, pd, v, e, wbb, wab, pe, pn, D)
        gv, ge, dwbb, dwab = conv.atom_bwd(ops, pd, saved, pe, pn, D, wbb,
                                           wab, go_v, go_e)
        outs[n_pack] = (v2h, e2h, gv, ge, dwbb, dwab)
        for got, ref in zip(outs[n_pack], want):
            assert (got - ref).abs().max().item() < 1e-11
    for a, b in zip(outs[4], outs[5]):
        assert torch.equal(a, b)

    # the options of the new block: saves handed over as a list are
    # consumed, and need_gv=False leaves everything else as it was
    pe, pn = _packed_weights(m_e), _packed_weights(m_n)
    v2n, e2n, saved = conv.atom_fwd(ops, pd, v, e, wbb, wab, pe, pn, D,
                                    saves_only=True)
    assert v2n is None and e2n is None
    saved = list(saved)
    gv, ge, dwbb, dwab = conv.atom_bwd(ops, pd, saved, pe, pn, D, wbb, wab,
                                       go_v, go_e, need_gv=False)
    assert gv is None and saved == []
    for got, ref in zip((ge, dwbb, dwab), outs[5][3:]):
        assert torch.equal(got, ref)
