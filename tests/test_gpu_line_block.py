"""GPU tests of the self-recomputing line-graph blocks (conv._BondBlockFn,
conv._AngleBlockFn), the default of checkpointed steps without a bond mask:
outputs and gradients against the op-by-op bodies of runtime under a
non-reentrant torch.utils.checkpoint (what they replace) and against fp64
plain torch, the l_dst segment sums of the bond block's reverse tail against
the r_seg_ldst launch, and through SpmdEngine(checkpoint="on") with the
DM_NO_LINE_BLOCK=1 switch.

The graph is the project's builder on a jittered diamond-Si cell of 360 atoms,
periodic along x only (cutoffs 6 / 3 A): the surfaces leave bonds without an
incoming line edge, L is no multiple of 32 and l_dst segments cross tile
boundaries.

Accuracy bound of the gradients and forces: max |err| against fp64 at most 2x
that of the op-by-op path on the same inputs (tests/test_gpu_atom_block.py);
of the segment sums: 1 ulp from the two-kernel path
(tests/test_gpu_fused_seg.py)."""
import copy
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_fused_seg import _ordered  # noqa: E402
from test_gpu_mlp_tail_bwd import D, _bound, _mlp  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs HIP GPU")

N_RBF = 9


def _structure():
    from distmlip_amd.structures import diamond_si
    s = diamond_si((5, 3, 3), jitter=0.1, seed=3)
    return dataclasses.replace(s, pbc=np.array([1, 0, 0], dtype=np.int64))


@pytest.fixture(scope="module")
def graph():
    """(pd on the GPU for HipOps, pd on the CPU for the fp64 reference)."""
    from distmlip_amd.chgnet import PartitionData
    from distmlip_amd.dist import Distributed
    s = _structure()
    dist = Distributed.create_distributed(
        s.cart_coords, s.frac_coords, s.lattice, 1, s.pbc, 6.0, 3.0,
        use_bond_graph=True, num_threads=2)
    pd = PartitionData(dist, 0, "cuda:0", True)
    pr = PartitionData(dist, 0, "cpu", True)
    L, rp = len(pr.l_dst), pd.line_row_ptr.cpu().long()
    assert L % 32 != 0, L
    deg = rp[1:] - rp[:-1]
    assert int((deg == 0).sum()) > 0, "every bond has an incoming line edge"
    first, last = rp[:-1][deg > 0], rp[1:][deg > 0] - 1
    assert int(((first >> 5) != (last >> 5)).sum()) > 0, \
        "no l_dst segment crosses a tile boundary"
    return pd, pr


class _Case:
    def __init__(self, pd):
        dev = pd.l_src.device
        gen = torch.Generator(device="cpu").manual_seed(505)

        def rnd(*shape):
            return torch.randn(*shape, generator=gen).to(dev)

        B, L, N = pd.n_bonds, len(pd.l_src), pd.n_atoms
        self.n, self.a, self.v = rnd(B, D), rnd(L, D), rnd(N, D)
        self.exp3, self.W3 = rnd(B, N_RBF), rnd(D, N_RBF) / 3
        self.go_n, self.go_a = rnd(B, D), rnd(L, D)
        self.bond_mlp, self.angle_mlp = _mlp(4, dev, 61), _mlp(4, dev, 62)


@pytest.fixture(scope="module")
def case(graph):
    return _Case(graph[0])


def _run(case, pd, ops, dtype, kind, mode):
    """kind "bond": (n2, dn, da, dv, dexp3); "angle": (a2, dn, da, dv).
    mode: "block" (the Function), "ckpt" (runtime's op-by-op body under a
    non-reentrant checkpoint), "plain" (the body alone)."""
    from distmlip_amd.chgnet import _packed_weights, gated_mlp_split4
    from distmlip_amd.conv import _AngleBlockFn, _BondBlockFn
    c, dev = case, pd.l_src.device
    n, a, v, exp3 = (t.detach().to(dev, dtype).clone().requires_grad_(True)
                     for t in (c.n, c.a, c.v, c.exp3))
    W3 = c.W3.to(dev, dtype)
    mlp = copy.deepcopy(c.bond_mlp if kind == "bond" else c.angle_mlp).to(
        dev, dtype)

    def bond_body(n_, a_, v_, e3):
        w3 = torch.nn.functional.linear(e3, W3)
        wl = ops.gather(w3, pd.l_src, csr=pd.line_src_csr)
        msg = gated_mlp_split4(mlp, n_, a_, v_, pd, ops, D, w=wl)
        return ops.scatter_lines(msg, pd, base=n_)

    def angle_body(n_, a_, v_):
        return gated_mlp_split4(mlp, n_, a_, v_, pd, ops, D, base=a_)

    if kind == "bond":
        body, args = bond_body, (n, a, v, exp3)
        go = c.go_n
    else:
        body, args = angle_body, (n, a, v)
        go = c.go_a
    if mode == "block" and kind == "bond":
        out = _BondBlockFn.apply(n, a, v, exp3, W3, pd, ops,
                                 _packed_weights(mlp), D)
    elif mode == "block":
        out = _AngleBlockFn.apply(n, a, v, pd, ops, _packed_weights(mlp), D)
    elif mode == "ckpt":
        out = torch.utils.checkpoint.checkpoint(body, *args,
                                                use_reentrant=False)
    else:
        out = body(*args)
    (out * go.to(dev, dtype)).sum().backward()
    return (out.detach(),) + tuple(t.grad for t in args)


NAMES = ("out", "dn", "da", "dv", "dexp3")


@requires_gpu
@pytest.mark.parametrize("kind", ["bond", "angle"])
def test_block_vs_checkpoint_and_fp64(monkeypatch, graph, case, kind):
    from distmlip_amd import mlp_path
    from distmlip_amd.ops import HipOps
    from oracle.chgnet_ref import CpuRefOps
    pd, pr = graph
    for name in list(mlp_path.SWITCHES) + [mlp_path.NO_FUSED_SEG,
                                           mlp_path.NO_LINE_BLOCK]:
        monkeypatch.delenv(name, raising=False)
    assert mlp_path.line_block(HipOps(), D)
    # the block's kernels: one no-keep whole-MLP launch outside, one keep
    # launch in the recomputation, one reverse tail, and no gathered [L,d]
    # copy of w3 or go_n2
    import distmlip_amd.ops as ops_mod
    calls = {"mlp": [], "tail": [], "gather": 0}
    real_mlp, real_tail = ops_mod.raw_gated_mlp, ops_mod.raw_mlp_tail_bwd
    real_gather = ops_mod.raw_gather

    def mlp_(*a, **k):
        calls["mlp"].append((a[9], k.get("w_idx") is not None
                             or (len(a) > 11 and a[11] is not None)))
        return real_mlp(*a, **k)

    def tail_(go, cg, w, z, w2, go_idx=None, seg=None, w_idx=None):
        calls["tail"].append((go_idx is not None, seg is not None,
                              w_idx is not None))
        return real_tail(go, cg, w, z, w2, go_idx, seg, w_idx)

    def gather_(*a):
        calls["gather"] += 1
        return real_gather(*a)

    monkeypatch.setattr(ops_mod, "raw_gated_mlp", mlp_)
    monkeypatch.setattr(ops_mod, "raw_mlp_tail_bwd", tail_)
    monkeypatch.setattr(ops_mod, "raw_gather", gather_)
    got = _run(case, pd, HipOps(), torch.float32, kind, "block")
    bond = kind == "bond"
    assert [k for k, _ in calls["mlp"]] == [False, True], calls
    assert calls["mlp"][0][1] == bond, calls
    assert calls["tail"] == [(bond, bond, bond)], calls
    assert calls["gather"] == 0, calls
    old = _run(case, pd, HipOps(), torch.float32, kind, "ckpt")
    ref = _run(case, pr, CpuRefOps(), torch.float64, kind, "plain")
    assert torch.equal(got[0], old[0]), f"{kind}: forward output differs"
    for name, g, o, r in zip(NAMES, got, old, ref):
        _bound(g.cpu(), r, o.cpu(), f"{kind} {name}")


@requires_gpu
def test_recomputation_is_the_outer_forward(graph, case):
    """bond_fwd / angle_fwd in their one-kernel keep form give the bits of the
    lean forwards (indexed or over the gathered wl), and the form without out
    keeps the same z and cg."""
    from distmlip_amd import conv
    from distmlip_amd.chgnet import _packed_weights
    from distmlip_amd.ops import HipOps
    pd, _ = graph
    c, ops = case, HipOps()
    pb, pa = _packed_weights(c.bond_mlp), _packed_weights(c.angle_mlp)
    with torch.no_grad():
        w3 = torch.nn.functional.linear(c.exp3, c.W3)
        n2, (z, cg, wl) = conv.bond_fwd(ops, pd, c.n, c.a, c.v, w3, pb, D)
        assert wl is None
        assert torch.equal(n2, conv._lean_bond(ops, pd, c.n, c.a, c.v, w3, pb,
                                               D, indexed=True))
        assert torch.equal(n2, conv._lean_bond(ops, pd, c.n, c.a, c.v, w3, pb,
                                               D))
        _, (z_s, cg_s, _) = conv.bond_fwd(ops, pd, c.n, c.a, c.v, w3, pb, D,
                                          saves_only=True)
        for x, y, what in ((z_s, z, "z"), (cg_s, cg, "cg")):
            assert torch.equal(x, y), what
        a2, (za, cga) = conv.angle_fwd(ops, pd, c.n, c.a, c.v, pa, D)
        assert torch.equal(a2, conv._lean_angle(ops, pd, c.n, c.a, c.v, pa,
                                                D))
        _, (za_s, cga_s) = conv.angle_fwd(ops, pd, c.n, c.a, c.v, pa, D,
                                          saves_only=True)
        for x, y, what in ((za_s, za, "z"), (cga_s, cga, "cg")):
            assert torch.equal(x, y), f"angle {what}"


@requires_gpu
def test_segment_sums(graph, case):
    """seg_ldst(dz) from the reverse tail's epilogue on the built line graph:
    at most 1 ulp from the r_seg_ldst launch, dz and dwl unchanged, bonds
    without line edges 0."""
    from distmlip_amd import conv
    from distmlip_amd.chgnet import _packed_weights
    from distmlip_amd.ops import HipOps, LineSeg
    pd, _ = graph
    c, ops = case, HipOps()
    pb = _packed_weights(c.bond_mlp)
    with torch.no_grad():
        w3 = torch.nn.functional.linear(c.exp3, c.W3)
        _, (z, cg, _) = conv.bond_fwd(ops, pd, c.n, c.a, c.v, w3, pb, D,
                                      saves_only=True)
        args = (c.go_n, cg, w3, z, pb[2], pd.l_dst)
        dz0, dw0 = ops.r_mlp_tail_bwd(*args, w_idx=pd.l_src)
        dz, dw, sums = ops.r_mlp_tail_bwd(*args, w_idx=pd.l_src,
                                          seg=LineSeg(pd))
        pair = ops.r_seg_ldst(dz0, pd)
    assert torch.equal(dz, dz0) and torch.equal(dw, dw0)
    off = (_ordered(sums) - _ordered(pair)).abs()
    print(f"line seg sums: differ {(off > 0).double().mean().item():.3e} of "
          f"elements, max {int(off.max())} ulp")
    assert int(off.max()) <= 1
    empty = pd.line_row_ptr[1:] == pd.line_row_ptr[:-1]
    assert not sums[empty].any()


CHAIN_NAMES = ("v2", "e3", "a2", "dv", "de", "dbexp", "da", "dexp3")


def _chain(case, pd, ops, dtype, plain=False):
    """Atom block, edge_to_bond, bond block, bond_to_edge, angle block, next
    atom block, wired as runtime.step wires a checkpointed step (one
    ExchangeHolder for the boundary where mlp_path.lazy_exchange holds; the
    line blocks where mlp_path.line_block holds, else their op-by-op bodies
    under a non-reentrant checkpoint).  plain: the op-by-op bodies and the two
    index_copy lines alone (the fp64 reference).  Returns (v2, e3, a2, dv, de,
    dbexp, da, dexp3) and the holder."""
    from distmlip_amd import conv, mlp_path
    from distmlip_amd.chgnet import (_packed_weights, gated_mlp_split3,
                                     gated_mlp_split4)
    c, dev = case, pd.l_src.device
    gen = torch.Generator(device="cpu").manual_seed(606)
    E, B = len(pd.src), pd.n_bonds

    def rnd(*shape):
        return torch.randn(*shape, generator=gen).to(dev, dtype)

    e0, bexp0 = rnd(E, D), rnd(E, N_RBF)
    Wbb, Wab, n_prev = rnd(D, N_RBF) / 3, rnd(D, N_RBF) / 3, rnd(B, D)
    go_v, go_e = rnd(pd.n_atoms, D), rnd(E, D)
    v, a, exp3 = (t.detach().to(dev, dtype).clone().requires_grad_(True)
                  for t in (c.v, c.a, c.exp3))
    e, bexp = e0.requires_grad_(True), bexp0.requires_grad_(True)
    W3 = c.W3.to(dev, dtype)
    atoms = [tuple(copy.deepcopy(_mlp(3, c.v.device, 71 + 2 * i + j)).to(
        dev, dtype) for j in range(2)) for i in range(2)]
    bond_mlp, angle_mlp = (copy.deepcopy(m).to(dev, dtype)
                           for m in (c.bond_mlp, c.angle_mlp))

    def atom_body(v_, e_, bexp_, m_e, m_n):
        wbb, wab = bexp_ @ Wbb.t(), bexp_ @ Wab.t()
        e2 = gated_mlp_split3(m_e, v_, e_, pd, ops, D, w=wbb, base=e_)
        msg = gated_mlp_split3(m_n, v_, e2, pd, ops, D, w=wab)
        return ops.scatter_edges(msg, pd, base=v_), e2

    def bond_body(n_, a_, v_, e3):
        w3 = torch.nn.functional.linear(e3, W3)
        wl = ops.gather(w3, pd.l_src, csr=pd.line_src_csr)
        msg = gated_mlp_split4(bond_mlp, n_, a_, v_, pd, ops, D, w=wl)
        return ops.scatter_lines(msg, pd, base=n_)

    def angle_body(n_, a_, v_):
        return gated_mlp_split4(angle_mlp, n_, a_, v_, pd, ops, D, base=a_)

    def ck(fn, *args):
        return torch.utils.checkpoint.checkpoint(fn, *args,
                                                 use_reentrant=False)

    holder = None
    if plain:
        v1, e1 = atom_body(v, e, bexp, *atoms[0])
        n = n_prev.index_copy(0, pd.map_ude, e1[pd.map_de])
        n2 = bond_body(n, a, v1, exp3)
        e2 = e1.index_copy(0, pd.map_de, n2[pd.map_ude])
        a2 = angle_body(n2, a, v1)
        v2, e3 = atom_body(v1, e2, bexp, *atoms[1])
    else:
        packs = [tuple(_packed_weights(m) for m in pair) for pair in atoms]
        if mlp_path.lazy_exchange(ops, D):
            holder = conv.ExchangeHolder()
        v1, e1 = conv._AtomBlockFn.apply(v, e, bexp, Wbb, Wab, None, pd, ops,
                                         *packs[0], D, holder)
        e1, n = conv.edge_to_bond(e1, n_prev, pd, ops, holder)
        line = conv.line_block_available(ops, _packed_weights(bond_mlp), D,
                                         dtype)
        if line:
            n2 = conv._BondBlockFn.apply(n, a, v1, exp3, W3, pd, ops,
                                         _packed_weights(bond_mlp), D)
        else:
            n2 = ck(bond_body, n, a, v1, exp3)
        e2 = conv.bond_to_edge(e1, n2, pd, ops, holder)
        if line:
            a2 = conv._AngleBlockFn.apply(n2, a, v1, pd, ops,
                                          _packed_weights(angle_mlp), D)
        else:
            a2 = ck(angle_body, n2, a, v1)
        v2, e3 = conv._AtomBlockFn.apply(v1, e2, bexp, Wbb, Wab, None, pd, ops,
                                         *packs[1], D)
    ((v2 * go_v).sum() + (e3 * go_e).sum()
     + (a2 * c.go_a.to(dev, dtype)).sum()).backward()
    return (v2.detach(), e3.detach(), a2.detach(), v.grad, e.grad, bexp.grad,
            a.grad, exp3.grad), holder


@requires_gpu
def test_chain_with_lazy_exchange(monkeypatch, graph, case):
    """The chain of a checkpointed step around one edge/bond boundary with
    the lazy exchange on: the line blocks against the same chain with
    DM_NO_LINE_BLOCK=1.  The holder is bound and block k reads the exchanged
    rows through r_edge_mlp_bwd's patch in both; the forward outputs are
    equal; the v, e, bexp, a and exp3 gradients hold the bound of the module
    docstring against the fp64 plain-torch chain (the two differ in the order
    of fp32 sums in the line blocks' reverse only)."""
    from distmlip_amd import mlp_path
    from distmlip_amd.ops import HipOps
    from oracle.chgnet_ref import CpuRefOps
    pd, pr = graph
    for name in list(mlp_path.SWITCHES) + [mlp_path.NO_FUSED_SEG,
                                           mlp_path.NO_LINE_BLOCK,
                                           mlp_path.NO_LAZY_EXCHANGE]:
        monkeypatch.delenv(name, raising=False)
    patched = []
    real_bwd = HipOps.r_edge_mlp_bwd

    def bwd(self, *a, patch=None, **k):
        patched.append(patch is not None)
        return real_bwd(self, *a, patch=patch, **k)

    monkeypatch.setattr(HipOps, "r_edge_mlp_bwd", bwd)
    from distmlip_amd import conv
    reverses = []
    for name in ("bond_bwd", "angle_bwd"):
        real = getattr(conv, name)
        monkeypatch.setattr(
            conv, name, lambda *a, _r=real, _n=name, **k: (
                reverses.append(_n), _r(*a, **k))[1])

    def run(line):
        del patched[:], reverses[:]
        assert mlp_path.lazy_exchange(HipOps(), D)
        out, holder = _chain(case, pd, HipOps(), torch.float32)
        assert holder is not None and holder.bound and not holder.pending
        assert sum(patched) == 1, "block k did not read the patch"
        assert reverses == (["angle_bwd", "bond_bwd"] if line else []), \
            reverses
        return out

    assert mlp_path.line_block(HipOps(), D)
    new = run(True)
    monkeypatch.setenv("DM_NO_LINE_BLOCK", "1")
    assert not mlp_path.line_block(HipOps(), D)
    old = run(False)
    monkeypatch.delenv("DM_NO_LINE_BLOCK")
    ref, _ = _chain(case, pr, CpuRefOps(), torch.float64, plain=True)
    for name, g, o in zip(CHAIN_NAMES[:3], new, old):
        assert torch.equal(g, o), f"chain {name} differs under the switch"
    differ = 0
    for name, g, o, r in zip(CHAIN_NAMES, new, old, ref):
        _bound(g.cpu(), r, o.cpu(), f"chain {name}")
        differ += not torch.equal(g, o)
    print(f"chain: {differ} of 5 gradients differ in bits under the switch")


@requires_gpu
def test_engine_checkpointed(monkeypatch):
    """SpmdEngine(checkpoint="on") on the cell: the default takes the blocks
    for every bond and angle update, DM_NO_LINE_BLOCK=1 for none; the energy
    is equal and the forces hold the bound against the fp64 oracle."""
    from distmlip_amd import conv
    from distmlip_amd.model import CHGNetCore
    from distmlip_amd.runtime import SpmdEngine
    from oracle.chgnet_ref import oracle_forward
    from oracle.graph_ref import brute_force_neighbors
    s = _structure()
    core = CHGNetCore.seeded(seed=0).float()
    core64 = copy.deepcopy(core).double()
    nb = len(core.atom_convs)
    g = brute_force_neighbors(s.frac_coords, s.lattice, s.pbc, 6.0, 3.0)
    ref = oracle_forward(core64, s, g["src"], g["dst"], g["offsets"],
                         g["within_bond_r"], dtype=torch.float64)
    applies = {"bond": 0, "angle": 0}
    for key, fn in (("bond", conv._BondBlockFn), ("angle", conv._AngleBlockFn)):
        real = fn.forward

        def fwd(*a, _real=real, _key=key):
            applies[_key] += 1
            return _real(*a)

        monkeypatch.setattr(fn, "forward", staticmethod(fwd))

    def run():
        eng = SpmdEngine(core, world=1, threads=2, device="cuda:0",
                         checkpoint="on")
        out = eng.step(s)
        F = np.zeros((s.num_atoms, 3))
        F[out["global_ids_owned"]] = \
            out["forces_owned"].double().cpu().numpy()
        return out["energy"].item(), torch.from_numpy(F)

    monkeypatch.delenv("DM_NO_LINE_BLOCK", raising=False)
    E_new, F_new = run()
    assert applies == {"bond": nb - 1, "angle": nb - 2}, applies
    monkeypatch.setenv("DM_NO_LINE_BLOCK", "1")
    E_old, F_old = run()
    assert applies == {"bond": nb - 1, "angle": nb - 2}, \
        "DM_NO_LINE_BLOCK=1 still took the block path"
    assert E_new == E_old, (E_new, E_old)
    _bound(F_new, ref["forces"].double(), F_old, "engine forces")
