"""GPU tests of the reverse gated-MLP tail with the dst segment sums of dz in
its epilogue (dm_gated_mlp_tail_bwd_seg_f32: k_gated_mlp_tail_bwd_seg +
k_seg_fixup), against the pair it replaces: the existing reverse-tail entry
followed by dm_seg_sum_f32 over its dz.

dz and dw / dbexp must be the existing entry's bit for bit.  The sums may
differ from dm_seg_sum_f32's by at most 1 fp32 ulp per element (a node
spread over several 32-row tiles gets a reassociated fp64 sum; a node within
one tile the same fp64 order, hence the same bits), and the share of elements
that differ at all is printed.  Against a torch fp64 sum the fused path's
largest error, in ulps of the reference, may exceed the pair's by at most 1.

Only the reverse tail is fused, and it takes no base: the forward tail and
r_seg_dst's base argument keep the two-kernel path."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_mlp_tail_bwd import D, _csr_of, _mlp, _packs  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs HIP GPU")

N_RBF = 9
DEGREES = (0, 1, 2, 46, 70, 200)
E_CASES = [1, 31, 32, 33, 2049]


def _graph(degrees, dev, E=None):
    """dst-sorted rows for the given node degrees, cut off after E rows."""
    deg = torch.tensor(degrees, dtype=torch.int64)
    if E is not None:
        cum = torch.cumsum(deg, 0)
        deg = torch.minimum(deg, (E - (cum - deg)).clamp(min=0))
    dst = torch.repeat_interleave(torch.arange(len(deg)), deg)
    rp = torch.zeros(len(deg) + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(deg, 0)
    return types.SimpleNamespace(
        dst=dst.to(torch.int32).to(dev), row_ptr=rp.to(torch.int32).to(dev),
        n_atoms=len(deg), E=int(rp[-1]))


def _mixed_degrees(n, seed):
    """Leading, trailing and a middle run of empty nodes around degrees drawn
    from DEGREES: segments inside a tile (several per tile at degree 1, 2),
    across one tile boundary (46), and over three or more tiles (70, 200)."""
    gen = torch.Generator().manual_seed(seed)
    pick = torch.randint(0, len(DEGREES), (n,), generator=gen)
    deg = [DEGREES[i] for i in pick.tolist()]
    mid = len(deg) // 2
    return [0, 0] + deg[:mid] + [0] * 5 + deg[mid:] + [0, 0, 0]


def _graphs(dev):
    gs = {f"E{E}": _graph(_mixed_degrees(40, E)[2:] + [200] * 12, dev, E)
          for E in E_CASES}
    gs["E1_lead"] = _graph([0, 0, 1, 0], dev)
    # exactly one tile per node, and nodes ending on every tile boundary
    gs["aligned"] = _graph([32, 32, 64, 0, 32, 16, 16, 96], dev)
    gs["ones"] = _graph([1] * 70, dev)         # 32 segments in a tile
    gs["mixed"] = _graph(_mixed_degrees(290, 7), dev)
    return gs


class _Data:
    def __init__(self):
        self.dev = dev = torch.device("cuda:0")
        self.graphs = _graphs(dev)
        assert [self.graphs[f"E{E}"].E for E in E_CASES] == E_CASES
        E = max(g.E for g in self.graphs.values())
        gen = torch.Generator(device="cpu").manual_seed(2718)

        def rnd(*shape):
            return torch.randn(*shape, generator=gen).to(dev)

        self.go, self.cg, self.z = rnd(E, D), rnd(2, E, D), rnd(E, 2 * D)
        self.w, self.w2 = rnd(E, D), rnd(2, D, D) / 8
        self.go_tab = rnd(300, D)
        self.bexp, self.W = rnd(E, N_RBF), rnd(D, N_RBF) / 3
        self.mask = (torch.rand(E, generator=gen) < 0.7).float().to(dev)
        self.dbexp_in = rnd(E, N_RBF)


@pytest.fixture(scope="module")
def data():
    return _Data()


def _ordered(x):
    """fp32 bits as integers that count ulps across zero"""
    i = x.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def _ulps_off(x, ref64):
    """|x - ref| in units of the fp32 spacing at ref"""
    r32 = ref64.float()
    spacing = (torch.nextafter(r32.abs(), torch.full_like(r32, float("inf")))
               - r32.abs()).double()
    return ((x.double() - ref64).abs() / spacing).max().item()


def _check_sums(sums, dz, g, what):
    from distmlip_amd.ops import raw_seg_sum
    pair = raw_seg_sum(dz, g.row_ptr, g.n_atoms)
    ref = torch.zeros(g.n_atoms, 2 * D, dtype=torch.float64, device=dz.device)
    ref.index_add_(0, g.dst.long(), dz.double())
    off = (_ordered(sums) - _ordered(pair)).abs()
    share = (off > 0).double().mean().item()
    u_f, u_p = _ulps_off(sums, ref), _ulps_off(pair, ref)
    print(f"{what}: E={g.E} N={g.n_atoms} differ {share:.3e} of elements, "
          f"max {int(off.max())} ulp; vs fp64: fused {u_f:.3f} ulp, "
          f"pair {u_p:.3f} ulp")
    assert int(off.max()) <= 1, f"{what}: {int(off.max())} ulp from the pair"
    assert u_f <= u_p + 1.0, f"{what}: fused {u_f} ulp vs pair {u_p} ulp"
    empty = (g.row_ptr[1:] == g.row_ptr[:-1])
    assert not sums[empty].any(), f"{what}: a node without rows is not 0"


GRAPH_NAMES = [f"E{E}" for E in E_CASES] + ["E1_lead", "aligned", "ones",
                                            "mixed"]


@requires_gpu
@pytest.mark.parametrize("name", GRAPH_NAMES)
@pytest.mark.parametrize("indexed", [False, True])
def test_dense_w(data, indexed, name):
    from distmlip_amd.ops import raw_mlp_tail_bwd
    d, g = data, data.graphs[name]
    E = g.E
    go, idx = (d.go_tab, g.dst) if indexed else (d.go[:E], None)
    args = (go, d.cg[:, :E].contiguous(), d.w[:E], d.z[:E], d.w2, idx)
    dz0, dw0 = raw_mlp_tail_bwd(*args)
    dz, dw, sums = raw_mlp_tail_bwd(*args, seg=g)
    assert torch.equal(dz, dz0) and torch.equal(dw, dw0)
    _check_sums(sums, dz0, g, f"dense idx={indexed} {name}")


@requires_gpu
@pytest.mark.parametrize("name", GRAPH_NAMES)
@pytest.mark.parametrize("indexed,masked,acc", [
    (False, True, True), (True, False, False), (True, True, True),
    (False, False, False)])
def test_factored_w(data, indexed, masked, acc, name):
    from distmlip_amd.ops import RadialW, raw_mlp_tail_bwd
    d, g = data, data.graphs[name]
    E = g.E
    go, idx = (d.go_tab, g.dst) if indexed else (d.go[:E], None)

    def rw(seg):
        return RadialW(d.bexp[:E], d.W, d.mask[:E] if masked else None,
                       d.dbexp_in[:E].clone() if acc else None, seg)

    args = (d.z[:E], d.w2, idx)
    cg = d.cg[:, :E].contiguous()
    dz0, db0 = raw_mlp_tail_bwd(go, cg, rw(None), *args)
    dz, db, sums = raw_mlp_tail_bwd(go, cg, rw(g), *args)
    assert torch.equal(dz, dz0) and torch.equal(db, db0)
    _check_sums(sums, dz0, g, f"factored idx={indexed} mask={masked} {name}")


def _atom_case(dev):
    """A 200-atom graph of about 20 neighbours, factored weights, two MLPs."""
    gen = torch.Generator(device="cpu").manual_seed(55)
    N, E = 200, 4001
    src = torch.randint(0, N, (E,), generator=gen)
    dst = torch.sort(torch.randint(0, N, (E,), generator=gen)).values
    pd = types.SimpleNamespace(n_atoms=N, src=src.to(torch.int32).to(dev),
                               dst=dst.to(torch.int32).to(dev))
    _, pd.row_ptr = _csr_of(dst, N, dev)
    pd.src_perm, pd.src_row_ptr = _csr_of(src, N, dev)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen).to(dev)

    t = types.SimpleNamespace(pd=pd, v=rnd(N, D), e=rnd(E, D),
                              bexp=rnd(E, N_RBF), Wbb=rnd(D, N_RBF) / 3,
                              Wab=rnd(D, N_RBF) / 3, go_v=rnd(N, D),
                              go_e=rnd(E, D))
    t.pe, t.pn = _packs(_mlp(3, dev, 61)), _packs(_mlp(3, dev, 62))
    return t


@requires_gpu
def test_switch_restores_the_seg_sum_launches(monkeypatch):
    """atom_bwd over factored weights: by default no r_seg_dst launch and
    both reverse tails return the sums; with DM_NO_FUSED_SEG=1 the two
    r_seg_dst launches and no RadialW that carries the graph, i.e. the calls
    made before the fusion.  ge and dbexp do not depend on the sums and are
    the same bits; gv moves by the sums' last bits only."""
    from distmlip_amd import conv
    from distmlip_amd.ops import HipOps, RadialW
    monkeypatch.delenv("DM_NO_FUSED_SEG", raising=False)
    t = _atom_case(torch.device("cuda:0"))
    ops = HipOps()
    calls = {"seg_dst": 0, "with_seg": 0}
    real_seg, real_tail = HipOps.r_seg_dst, HipOps.r_mlp_tail_bwd

    def seg_dst(self, *a, **k):
        calls["seg_dst"] += 1
        return real_seg(self, *a, **k)

    def tail(self, go, cg, w, *a):
        calls["with_seg"] += w.seg is not None
        return real_tail(self, go, cg, w, *a)

    monkeypatch.setattr(HipOps, "r_seg_dst", seg_dst)
    monkeypatch.setattr(HipOps, "r_mlp_tail_bwd", tail)

    def run():
        calls.update(seg_dst=0, with_seg=0)
        wbb, wab = RadialW(t.bexp, t.Wbb), RadialW(t.bexp, t.Wab)
        with torch.no_grad():
            saved = conv.atom_fwd(ops, t.pd, t.v, t.e, wbb, wab, t.pe, t.pn,
                                  D, saves_only=True)[2]
            out = conv.atom_bwd(ops, t.pd, list(saved), t.pe, t.pn, D, wbb,
                                wab, t.go_v, t.go_e)
        return out[:3], dict(calls)

    (gv, ge, db), n = run()
    assert n == {"seg_dst": 0, "with_seg": 2}, n
    monkeypatch.setenv("DM_NO_FUSED_SEG", "1")
    (gv0, ge0, db0), n0 = run()
    assert n0 == {"seg_dst": 2, "with_seg": 0}, n0
    assert torch.equal(ge, ge0) and torch.equal(db, db0)
    # gv = go_v + four [N,128] x [128,64] products of sums of |.| ~ 1e2;
    # a 1-ulp move of a few sums stays far below 1e-4 of that scale
    err = (gv - gv0).abs().max().item()
    print(f"gv: max |fused - switch| {err:.3e}, scale "
          f"{gv0.abs().max().item():.3e}")
    assert err <= 1e-4 * gv0.abs().max().item()
    # need_gv=False (a first block): no sums either way
    monkeypatch.delenv("DM_NO_FUSED_SEG")
    calls.update(seg_dst=0, with_seg=0)
    wbb, wab = RadialW(t.bexp, t.Wbb), RadialW(t.bexp, t.Wab)
    with torch.no_grad():
        saved = conv.atom_fwd(ops, t.pd, t.v, t.e, wbb, wab, t.pe, t.pn, D,
                              saves_only=True)[2]
        out = conv.atom_bwd(ops, t.pd, list(saved), t.pe, t.pn, D, wbb, wab,
                            t.go_v, t.go_e, need_gv=False)
    assert out[0] is None and calls == {"seg_dst": 0, "with_seg": 0}
    assert torch.equal(out[1], ge0) and torch.equal(out[2], db0)
