"""Hand-sequenced atom-conv block (forward + reverse pass as ONE autograd
Function).

Replaces autograd's op-by-op reverse for the atom-conv blocks
(reference layer structure: implementations/matgl/models/chgnet.py:300-313
twice per block — edge update then node update).  The math is identical
to chgnet.gated_mlp_split3 + scatter_edges; what changes is the reverse
pass: it is sequenced by hand over the backend's RAW primitives
(ops_base docstring), so every gradient accumulation lands as a fused
`addmm` / kernel `base` argument instead of autograd's separate
zero+copy+add passes (measured 12.6 ms/step of elementwise adds at
li100k, rocprof run 32 — the atom convs carry most of it).

Measured (run 36, same box): 141.6 vs 140.2 ms/step at li100k — the
earlier fixes (addmm-fused bias/grad chains, set_materialize_grads,
packed second layer) had already absorbed the accumulation passes this
targets inside the conv; the remaining eager adds live in the bond path
and the cross-conv chains.  Default is therefore OFF (DM_FUSED_CONV=1
opts in); the Function stays as tested infrastructure for the round-2
whole-graph reverse pass, and the SPMD gloo fp64 exactness tests pin it
against the oracle (both backends implement the raw primitives).

Checkpointed steps (si1m) take _AtomBlockFn instead: the same atom_fwd /
atom_bwd inside a node that recomputes itself, with the fused first layer,
its reverse kernel (gradient sums in the epilogue) and the indexed reverse
tail; 1205-1210 -> 1096-1102 ms/step at si1m (profiles/first_bwd_*).
Their final block keeps its saves (_AtomBlockKeepFn), and the 4M rows that
move between e and n around every bond block go through edge_to_bond /
bond_to_edge, in place over e (1011-1014 -> 909-914 ms/step,
profiles/row_exchange_*).
"""
from __future__ import annotations

import os

import torch


def _second_fwd(h, w2, b2, d):
    return torch.baddbmm(b2, h.view(-1, 2, d).transpose(0, 1), w2)


def _second_bwd(dcg, w2, d):
    """Two GEMMs writing STRIDED into one row-major dh (no re-pack copy)."""
    dcg = dcg.contiguous()
    dh = torch.empty(dcg.shape[1], 2 * d, dtype=dcg.dtype, device=dcg.device)
    torch.mm(dcg[0], w2[0].t(), out=dh[:, :d])
    torch.mm(dcg[1], w2[1].t(), out=dh[:, d:])
    return dh


def _mlp_tail_bwd(ops, go, cg, w, z, w2, d):
    """(dz, dw) from the gradient go of r_combine_fwd(cg, w, base): one
    kernel where the backend has r_mlp_tail_bwd (d = 64), else combine
    reverse + second-layer GEMMs + silu reverse.  DM_NO_FUSED_MLP_BWD=1
    forces the latter for A/B runs."""
    if (d == 64 and hasattr(ops, "r_mlp_tail_bwd")
            and os.environ.get("DM_NO_FUSED_MLP_BWD", "0") != "1"):
        return ops.r_mlp_tail_bwd(go, cg, w, z, w2)
    dcg, dw = ops.r_combine_bwd(go, cg, w)
    return ops.r_silu_bwd(_second_bwd(dcg, w2, d), z), dw


def _fused_tail_fwd(ops, d, name):
    return (d == 64 and hasattr(ops, name)
            and os.environ.get("DM_NO_FUSED_MLP_FWD", "0") != "1")


def _mlp_tail_fwd(ops, h, w2, b2, w, base, d):
    """(cg, out) with cg = the second layer over h and out =
    r_combine_fwd(cg, w, base): one kernel where the backend has
    r_mlp_tail_fwd (d = 64), else baddbmm + combine.  DM_NO_FUSED_MLP_FWD=1
    forces the latter for A/B runs."""
    if _fused_tail_fwd(ops, d, "r_mlp_tail_fwd"):
        return ops.r_mlp_tail_fwd(h, w2, b2, w, base)
    cg = _second_fwd(h, w2, b2, d)
    return cg, ops.r_combine_fwd(cg, w, base)


def _mlp_tail_act(ops, h, w2, b2, w, base, d):
    """out of _mlp_tail_fwd alone, for the save-nothing forwards: no cg is
    written where the backend has mlp_tail_act."""
    records = torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in (h, w, base))
    if not records and _fused_tail_fwd(ops, d, "mlp_tail_act"):
        return ops.mlp_tail_act(h, w2, b2, w, base)
    return ops.gated_combine_packed(_second_fwd(h, w2, b2, d), w, base)


def _unpack_edge(packs, d):
    wcg, bcg, w2, b2 = packs[:4]
    return wcg[:, :d], wcg[:, d:2 * d], wcg[:, 2 * d:], bcg, w2, b2


def _fusedT(packs):
    """The [d,2d] fusedT pack of a 5-element pack, None for a 4-pack."""
    return packs[4] if len(packs) > 4 else None


def _fused_first(ops, packs, d):
    """fusedT when the first layer can run as r_edge_mlp3 (5-pack, d = 64,
    a backend that has it), else None.  DM_NO_FUSED_MLP=1 forces None."""
    if (d == 64 and hasattr(ops, "r_edge_mlp3")
            and os.environ.get("DM_NO_FUSED_MLP", "0") != "1"):
        return _fusedT(packs)
    return None


def _fused_first_bwd(ops, packs, d):
    """fusedT when the first layer's reverse can run as r_edge_mlp_bwd,
    else None.  DM_NO_FUSED_MLP1_BWD=1 forces None (addmm, r_gather_dst)."""
    if (d == 64 and hasattr(ops, "r_edge_mlp_bwd")
            and os.environ.get("DM_NO_FUSED_MLP1_BWD", "0") != "1"):
        return _fusedT(packs)
    return None


def _first_fwd(ops, pd, v, e, packs, d):
    """(z, h) of one MLP's first layer over cat(v[src], v[dst], e)."""
    ws, wd, we, bcg, _, _ = _unpack_edge(packs, d)
    ft = _fused_first(ops, packs, d)
    if ft is not None:
        return ops.r_edge_mlp3(e, ft, bcg, v @ ws.t(), v @ wd.t(), pd)
    return ops.r_gather_add3(v @ ws.t(), v @ wd.t(),
                             torch.addmm(bcg, e, we.t()), pd)


def _fused_full(ops, d, name):
    """Whether a whole gated MLP can run as the one-kernel primitive `name`
    (first layer, second layer and combine, no h array): d = 64 and a backend
    that has it.  DM_NO_FUSED_MLP_FULL=1 restores the first-layer + tail
    kernel pair; the switches of those two kernels (DM_NO_FUSED_MLP,
    DM_NO_FUSED_MLP_FWD) turn it off as well."""
    return (_fused_tail_fwd(ops, d, name)
            and os.environ.get("DM_NO_FUSED_MLP", "0") != "1"
            and os.environ.get("DM_NO_FUSED_MLP_FULL", "0") != "1")


def _records(*ts):
    return torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in ts)


def _mlp_fwd(ops, pd, v, ebox, packs, w, base, d, want_out=True):
    """(z, cg, out) of one atom-graph gated MLP in keep form: one kernel
    where the backend has r_gated_mlp3 (5-pack, d = 64), else the first
    layer followed by the tail.  ebox is a one-element list holding the
    MLP's e rows.  want_out=False: out is not needed.  The one-kernel form
    then neither computes it nor reads w and base; the two-kernel path
    empties ebox once the first layer has read the rows, so that a caller
    who dropped its own reference has them freed before the tail."""
    ws, wd, _, bcg, w2, b2 = _unpack_edge(packs, d)
    ft = _fusedT(packs) if _fused_full(ops, d, "r_gated_mlp3") else None
    if ft is not None:
        return ops.r_gated_mlp3(ebox[0], ft, bcg, v @ ws.t(), v @ wd.t(), pd,
                                w2, b2, w, base, want_out)
    z, h = _first_fwd(ops, pd, v, ebox[0], packs, d)
    if not want_out:
        del ebox[:]
    cg, out = _mlp_tail_fwd(ops, h, w2, b2, w, base, d)
    return z, cg, out if want_out else None


def atom_fwd(ops, pd, v, e, wbb, wab, packs_edge, packs_node, d,
             saves_only=False):
    """One atom-conv block forward (chgnet.py:300-313 semantics).
    Returns (v2, e2, saved) with saved = (z1, cg1, z2, cg2).  Packs are
    (wcg, bcg, w2, b2[, fusedT]); with fusedT and a backend that has
    r_gated_mlp3 each MLP is one kernel, with r_edge_mlp3 alone the first
    layers are.  saves_only=True (a recomputation) returns (None, None,
    saved): msg is not needed, so the node MLP runs without out (one kernel)
    or has e2 freed before its tail (two), where a checkpointed step has
    its memory peak, and the segment sum is skipped."""
    z1, cg1, e2 = _mlp_fwd(ops, pd, v, [e], packs_edge, wbb, e, d)
    ebox = [e2]
    if saves_only:
        e2 = None
    z2, cg2, msg = _mlp_fwd(ops, pd, v, ebox, packs_node, wab, None, d,
                            want_out=not saves_only)
    v2 = ops.r_seg_dst(msg, pd, base=v) if not saves_only else None
    return v2, e2, (z1, cg1, z2, cg2)


def atom_bwd(ops, pd, saved, packs_edge, packs_node, d, wbb, wab,
             go_v2, go_e2, acc_wbb=None, acc_wab=None, need_gv=True):
    """Hand-sequenced reverse of atom_fwd.  Returns (gv, ge, dwbb, dwab), or
    with factored wbb / wab (ops.RadialW) (gv, ge, dbexp, None), dbexp being
    the gradient of their common bexp through both weights;
    with acc_wbb/acc_wab buffers the shared-weight grads are ACCUMULATED
    in place (add_) and None returned for them — the cross-block
    accumulation autograd would do with separate elementwise add
    passes.

    With 5-packs and a backend that has r_edge_mlp_bwd, the two per-edge
    reverse GEMMs and the sums they feed are one kernel each, and the
    node MLP's tail reads go_v2 by pd.dst instead of a gathered copy.
    saved may be a list: it is emptied, so each save is freed as soon as
    it is consumed.  need_gv=False skips the four segment sums and GEMMs
    of the v gradient (gv is None) when v takes no gradient."""
    z1, cg1, z2, cg2 = saved
    if isinstance(saved, list):
        saved.clear()
    factored = _is_factored(wbb)
    assert not factored or (acc_wbb is None and acc_wab is None)
    ws1, wd1, we1, _, w21, _ = _unpack_edge(packs_edge, d)
    ws2, wd2, we2, _, w22, _ = _unpack_edge(packs_node, d)
    ft1 = _fused_first_bwd(ops, packs_edge, d)
    ft2 = _fused_first_bwd(ops, packs_node, d)
    go_v2 = go_v2.contiguous() if go_v2 is not None else None
    go_e2 = go_e2.contiguous() if go_e2 is not None else None

    # node MLP reverse (v2 = v + seg_dst(msg))
    if go_v2 is not None:
        if (ft2 is not None and getattr(ops, "tail_bwd_indexed", False)
                and os.environ.get("DM_NO_FUSED_MLP_BWD", "0") != "1"):
            dz2, dwab = ops.r_mlp_tail_bwd(go_v2, cg2, wab, z2, w22,
                                           pd.dst)     # go_idx
        else:
            dmsg = ops.r_gather_dst(go_v2, pd)
            dz2, dwab = _mlp_tail_bwd(ops, dmsg, cg2, wab, z2, w22, d)
            del dmsg
        del z2, cg2
        # e2 grad: external + the node MLP's per-edge GEMM, fused.  The
        # result is a fresh buffer, never go_e2 itself
        if ft2 is not None:
            ge2 = ops.r_edge_mlp_bwd(dz2, ft2, go_e2)
        else:
            ge2 = (torch.addmm(go_e2, dz2, we2) if go_e2 is not None
                   else dz2 @ we2)
        owns_ge2 = True
    else:
        del z2, cg2
        dz2, dwab = None, None
        ge2 = go_e2
        owns_ge2 = False

    # edge MLP reverse (e2 = e + combine(cg1, wbb)).  Factored weights: the
    # node MLP's launch returned its dbexp in dwab; this launch adds its own
    # onto it in place, and the sum is returned as dwbb
    if factored and dwab is not None:
        wbb = wbb.with_acc(dwab)
        dwab = None
    dz1, dwbb = _mlp_tail_bwd(ops, ge2, cg1, wbb, z1, w21, d)
    del z1, cg1
    # base passthrough + GEMM; in place only over the ge2 made above
    if ft1 is not None:
        ge = ops.r_edge_mlp_bwd(dz1, ft1, ge2,
                                out=ge2 if owns_ge2 else None)
    else:
        ge = torch.addmm(ge2, dz1, we1)
    del ge2
    if need_gv:
        # v grad: passthrough + all four per-node GEMM backs, fused
        gv = torch.addmm(go_v2, ops.r_seg_src(dz1, pd), ws1) \
            if go_v2 is not None else ops.r_seg_src(dz1, pd) @ ws1
        gv.addmm_(ops.r_seg_dst(dz1, pd), wd1)
        del dz1
        if dz2 is not None:
            gv.addmm_(ops.r_seg_src(dz2, pd), ws2)
            gv.addmm_(ops.r_seg_dst(dz2, pd), wd2)
            del dz2
    else:
        gv = None
    if acc_wbb is not None:
        acc_wbb.add_(dwbb)
        dwbb = None
    if acc_wab is not None and dwab is not None:
        acc_wab.add_(dwab)
        dwab = None
    return gv, ge, dwbb, dwab


class _AtomConvFn(torch.autograd.Function):
    """(v, e) -> (v', e') for one atom-conv block, hand-written backward.

    packs = (wcg, bcg, w2, b2) per MLP from chgnet._packed_weights; all
    weights must be frozen (no weight grads are produced).  wbb/wab are
    the per-edge shared message weights (grad-carrying: they feed the
    force path through the radial expansions).
    """

    @staticmethod
    def forward(ctx, v, e, wbb, wab, pd, ops, packs_edge, packs_node, d):
        v2, e2, saved = atom_fwd(ops, pd, v, e, wbb, wab, packs_edge,
                                 packs_node, d)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*saved, wbb, wab)
        ctx.pd, ctx.ops, ctx.d = pd, ops, d
        ctx.packs = (packs_edge, packs_node)
        return v2, e2

    @staticmethod
    def backward(ctx, go_v2, go_e2):
        z1, cg1, z2, cg2, wbb, wab = ctx.saved_tensors
        pd, ops, d = ctx.pd, ctx.ops, ctx.d
        packs_edge, packs_node = ctx.packs
        with torch.no_grad():
            gv, ge, dwbb, dwab = atom_bwd(
                ops, pd, (z1, cg1, z2, cg2), packs_edge, packs_node, d,
                wbb, wab, go_v2, go_e2)
        return gv, ge, dwbb, dwab, None, None, None, None, None


def conv_fn_available(ops, mlp_pack) -> bool:
    """Hand-sequenced path policy: frozen weights, raw-primitive backend,
    recording mode, and explicit opt-in (measured ~1% slower than the
    op-by-op path after the addmm/materialize fixes — see module
    docstring)."""
    return (os.environ.get("DM_FUSED_CONV", "0") == "1"
            and hasattr(ops, "r_gather_add3")
            and not mlp_pack[0].requires_grad
            and torch.is_grad_enabled())


def bond_fwd(ops, pd, n, a, v, w3, packs, d, mask_l=None):
    """One bond (line-graph) node conv forward (chgnet.py:326-348).
    Returns (n2, saved) with saved = (z, cg, wl)."""
    wcg, bcg, w2, b2 = packs
    w1, wn2, wa, wv = (wcg[:, :d], wcg[:, d:2 * d], wcg[:, 2 * d:3 * d],
                       wcg[:, 3 * d:])
    wl = ops.r_gather_lsrc(w3, pd)
    if mask_l is not None:
        wl = wl * mask_l
    z, h = ops.r_gather_add4(n @ w1.t(), n @ wn2.t(),
                             torch.addmm(bcg, a, wa.t()), v @ wv.t(), pd)
    cg, msg = _mlp_tail_fwd(ops, h, w2, b2, wl, None, d)
    n2 = ops.r_seg_ldst(msg, pd, base=n)
    return n2, (z, cg, wl)


def bond_bwd(ops, pd, saved, packs, d, go_n2, mask_l=None,
             acc_w3=None, acc_a=None, acc_v=None):
    """Hand-sequenced reverse of bond_fwd.  Returns (gn, da, gv, gw3);
    da/gv/gw3 are accumulated into acc_* buffers (add_) when given."""
    z, cg, wl = saved
    wcg, _, w2, _ = packs
    w1, wn2, wa, wv = (wcg[:, :d], wcg[:, d:2 * d], wcg[:, 2 * d:3 * d],
                       wcg[:, 3 * d:])
    go_n2 = go_n2.contiguous()
    dmsg = ops.r_gather_ldst(go_n2, pd)
    dz, dwl = _mlp_tail_bwd(ops, dmsg, cg, wl, z, w2, d)
    if acc_a is not None:
        acc_a.addmm_(dz, wa)
        da = None
    else:
        da = dz @ wa
    gn = torch.addmm(go_n2, ops.r_seg_lsrc(dz, pd), w1)
    gn.addmm_(ops.r_seg_ldst(dz, pd), wn2)
    if acc_v is not None:
        acc_v.addmm_(ops.r_seg_center(dz, pd), wv)
        gv = None
    else:
        gv = ops.r_seg_center(dz, pd) @ wv
    if mask_l is not None:
        dwl = dwl * mask_l
    if acc_w3 is not None:
        acc_w3.add_(ops.r_seg_lsrc(dwl, pd))
        gw3 = None
    else:
        gw3 = ops.r_seg_lsrc(dwl, pd)
    return gn, da, gv, gw3


def angle_fwd(ops, pd, n, a, v, packs, d):
    """Angle (line-edge) update forward: a2 = a + GatedMLP(cat(n_lsrc,
    n_ldst, a, v_center)) (chgnet.py:350-368).  Returns (a2, saved)."""
    wcg, bcg, w2, b2 = packs
    w1, wn2, wa, wv = (wcg[:, :d], wcg[:, d:2 * d], wcg[:, 2 * d:3 * d],
                       wcg[:, 3 * d:])
    z, h = ops.r_gather_add4(n @ w1.t(), n @ wn2.t(),
                             torch.addmm(bcg, a, wa.t()), v @ wv.t(), pd)
    cg, a2 = _mlp_tail_fwd(ops, h, w2, b2, None, a, d)
    return a2, (z, cg)


def angle_bwd(ops, pd, saved, packs, d, go_a2, acc_n=None, acc_v=None):
    """Reverse of angle_fwd.  Returns (gn, da, gv); gn/gv accumulate into
    acc_* when given (da is the full pass-through + wa chain)."""
    z, cg = saved
    wcg, _, w2, _ = packs
    w1, wn2, wa, wv = (wcg[:, :d], wcg[:, d:2 * d], wcg[:, 2 * d:3 * d],
                       wcg[:, 3 * d:])
    go_a2 = go_a2.contiguous()
    dz, _ = _mlp_tail_bwd(ops, go_a2, cg, None, z, w2, d)
    da = torch.addmm(go_a2, dz, wa)
    if acc_n is not None:
        gn = None
        acc_n.addmm_(ops.r_seg_lsrc(dz, pd), w1)
        acc_n.addmm_(ops.r_seg_ldst(dz, pd), wn2)
    else:
        gn = ops.r_seg_lsrc(dz, pd) @ w1
        gn.addmm_(ops.r_seg_ldst(dz, pd), wn2)
    if acc_v is not None:
        acc_v.addmm_(ops.r_seg_center(dz, pd), wv)
        gv = None
    else:
        gv = ops.r_seg_center(dz, pd) @ wv
    return gn, da, gv


class _BondConvFn(torch.autograd.Function):
    """(n, a, v, w3) -> n' for one bond (line-graph) conv, hand-written
    backward (reference chgnet.py:326-368 semantics as orchestrated in
    runtime.bond_body).  mask_l ([L,1] detached, or None) is the verlet
    destination-bond mask applied to the line weights."""

    @staticmethod
    def forward(ctx, n, a, v, w3, pd, ops, packs, d, mask_l):
        n2, saved = bond_fwd(ops, pd, n, a, v, w3, packs, d, mask_l)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*saved)
        ctx.pd, ctx.ops, ctx.d = pd, ops, d
        ctx.packs = packs
        ctx.mask_l = mask_l
        return n2

    @staticmethod
    def backward(ctx, go_n2):
        z, cg, wl = ctx.saved_tensors
        with torch.no_grad():
            gn, da, gv, gw3 = bond_bwd(ctx.ops, ctx.pd, (z, cg, wl),
                                       ctx.packs, ctx.d, go_n2,
                                       mask_l=ctx.mask_l)
        return gn, da, gv, gw3, None, None, None, None, None


# ---------------------------------------------------------------------------
# Whole-graph hand-sequenced reverse (round-2)
# ---------------------------------------------------------------------------

def _lean_atom(ops, pd, v, e, wbb, wab, pe, pn, d):
    """Save-nothing atom-conv forward (recompute mode): the fused no-z
    first-layer kernel applies when available, exactly like the
    checkpointed op-by-op outer forward."""
    wcg1, bcg1, w21, b21, fusedT1 = pe
    wcg2, bcg2, w22, b22, fusedT2 = pn
    ws1, wd1 = wcg1[:, :d], wcg1[:, d:2 * d]
    ws2, wd2 = wcg2[:, :d], wcg2[:, d:2 * d]
    if d == 64 and hasattr(ops, "edge_mlp3_act"):
        h1 = ops.edge_mlp3_act(e, fusedT1, bcg1, v @ ws1.t(), v @ wd1.t(), pd)
    else:
        h1 = ops.gather_add3_act(v @ ws1.t(), v @ wd1.t(),
                                 torch.addmm(bcg1, e, wcg1[:, 2 * d:].t()),
                                 pd)
    e2 = _mlp_tail_act(ops, h1, w21, b21, wbb, e, d)
    if d == 64 and hasattr(ops, "edge_mlp3_act"):
        h2 = ops.edge_mlp3_act(e2, fusedT2, bcg2, v @ ws2.t(), v @ wd2.t(),
                               pd)
    else:
        h2 = ops.gather_add3_act(v @ ws2.t(), v @ wd2.t(),
                                 torch.addmm(bcg2, e2, wcg2[:, 2 * d:].t()),
                                 pd)
    msg = _mlp_tail_act(ops, h2, w22, b22, wab, None, d)
    return ops.scatter_edges(msg, pd, base=v), e2


def _block_w(bexp, W, edge_mask):
    """One shared message weight of a block: bexp @ W.t(), masked."""
    w = bexp @ W.t()
    return w if edge_mask is None else w * edge_mask


def _is_factored(w):
    return hasattr(w, "with_acc")        # ops.RadialW


def _factored_w(ops, bexp, d):
    """Whether a block hands its two message weights to the MLP tail kernels
    as factors (ops.RadialW: bexp, W, mask) instead of building the dense
    [E,d] arrays: a backend that takes them (fp32, d = 64, n_rbf = 9), and the
    fused tails in use.  DM_NO_FACTORED_W=1 restores the dense weights."""
    return (getattr(ops, "factored_w", False) and d == 64
            and bexp.dtype == torch.float32 and bexp.shape[1] == 9
            and os.environ.get("DM_NO_FACTORED_W", "0") != "1"
            and os.environ.get("DM_NO_FUSED_MLP_FWD", "0") != "1"
            and os.environ.get("DM_NO_FUSED_MLP_BWD", "0") != "1")


def _block_weights(ops, bexp, Wbb, Wab, edge_mask, d):
    """(wbb, wab) of a block: factored where _factored_w allows, else the two
    dense arrays of _block_w."""
    if _factored_w(ops, bexp, d):
        from .ops import RadialW
        bexp = bexp.detach().contiguous()
        mask = edge_mask.reshape(-1).contiguous() \
            if edge_mask is not None else None
        return (RadialW(bexp, Wbb.contiguous(), mask),
                RadialW(bexp, Wab.contiguous(), mask))
    return _block_w(bexp, Wbb, edge_mask), _block_w(bexp, Wab, edge_mask)


class _AtomBlockFn(torch.autograd.Function):
    """(v, e, bexp) -> (v', e') for one atom-conv block of a checkpointed
    step: a self-recomputing node in place of torch.utils.checkpoint around
    the op-by-op block.

    A Function.forward cannot tell a checkpoint's outer pass from its
    recomputation, so under the generic checkpoint the outer pass writes z
    and cg of both MLPs only to have them dropped, and the two gradients of
    e (erow of an MLP, and base / the next block's input) meet in an
    elementwise add between autograd nodes.  Here the forward is the
    save-nothing _lean_atom (no z, no cg) and keeps only v, e, bexp; the
    backward recomputes the block once in keep form (all at once, as the
    checkpoint did) and runs the hand-sequenced atom_bwd, where those sums
    are the epilogue of r_edge_mlp_bwd.

    Where the backend takes factored weights (_factored_w) the two shared
    message weights are never built: the tail kernels get bexp, Wbb / Wab and
    the mask and compute w in place, and the reverse tails return dbexp
    directly instead of two dense [E,d] gradients folded by two GEMMs.

    Wbb / Wab are the [d, n_rbf] weights of the bias-free shared message
    linears and must be frozen, like the packs pe / pn (5-element, from
    chgnet._packed_weights); edge_mask is the detached [E,1] verlet mask
    or None.
    """

    @staticmethod
    def forward(ctx, v, e, bexp, Wbb, Wab, edge_mask, pd, ops, pe, pn, d):
        assert not (Wbb.requires_grad or Wab.requires_grad
                    or pe[0].requires_grad or pn[0].requires_grad)
        wbb, wab = _block_weights(ops, bexp, Wbb, Wab, edge_mask, d)
        ctx.set_materialize_grads(False)
        ctx.consts = (Wbb, Wab, edge_mask, pd, ops, pe, pn, d)
        ctx.kept = None
        if getattr(ctx, "keep", False):
            # _AtomBlockKeepFn: the keep-form forward the backward would
            # have re-run.  z and cg are neither inputs nor outputs; they
            # hang on ctx as a plain list, which atom_bwd empties as it
            # goes, so each is freed once consumed (saved tensors would
            # all live until the backward returns)
            v2, e2, saved = atom_fwd(ops, pd, v.detach(), e.detach(), wbb,
                                     wab, pe, pn, d)
            ctx.kept = list(saved)
            ctx.save_for_backward(bexp)
            return v2, e2
        # grad mode is off here, but v and e still carry requires_grad, by
        # which the first-layer Function decides whether to store z:
        # detached, both MLPs take the no-z form
        v2, e2 = _lean_atom(ops, pd, v.detach(), e.detach(), wbb, wab, pe,
                            pn, d)
        ctx.save_for_backward(v, e, bexp)
        return v2, e2

    @staticmethod
    def backward(ctx, go_v2, go_e2):
        Wbb, Wab, edge_mask, pd, ops, pe, pn, d = ctx.consts
        with torch.no_grad():
            if getattr(ctx, "keep", False):
                assert ctx.kept, "a keep block runs its backward once"
                bexp, = ctx.saved_tensors
                saved, ctx.kept = ctx.kept, None
                wbb, wab = _block_weights(ops, bexp, Wbb, Wab, edge_mask, d)
            else:
                v, e, bexp = ctx.saved_tensors
                wbb, wab = _block_weights(ops, bexp, Wbb, Wab, edge_mask, d)
                saved = list(atom_fwd(ops, pd, v, e, wbb, wab, pe, pn, d,
                                      saves_only=True)[2])
            gv, ge, dwbb, dwab = atom_bwd(
                ops, pd, saved, pe, pn, d, wbb, wab, go_v2, go_e2,
                need_gv=ctx.needs_input_grad[0])
            factored = _is_factored(wbb)
            del wbb, wab
            dbexp = None
            if factored:
                # the two tail launches produced it, mask applied
                dbexp = dwbb if ctx.needs_input_grad[2] else None
            elif ctx.needs_input_grad[2]:
                if edge_mask is not None:
                    dwbb = dwbb * edge_mask
                    dwab = dwab * edge_mask if dwab is not None else None
                dbexp = dwbb @ Wbb
                if dwab is not None:
                    dbexp.addmm_(dwab, Wab)
        return (gv, ge, dbexp, None, None, None, None, None, None, None,
                None)


class _AtomBlockKeepFn(_AtomBlockFn):
    """_AtomBlockFn for the FINAL atom block of a checkpointed step: its
    backward starts as soon as the readout is done, so dropping z / cg only
    to recompute them buys nothing.  The forward runs in keep form (atom_fwd,
    same packs and factored weights, outputs bit for bit the lean form's)
    and the backward goes straight to atom_bwd.  Same arguments; it runs
    through _AtomBlockFn.forward with a flag on ctx."""

    @staticmethod
    def forward(ctx, *args):
        ctx.keep = True
        return _AtomBlockFn.forward(ctx, *args)


def final_keep_enabled() -> bool:
    """DM_NO_FINAL_KEEP=1 gives the final block back its recomputation."""
    return os.environ.get("DM_NO_FINAL_KEEP", "0") != "1"


# ---------------------------------------------------------------------------
# edge <-> bond row exchange of a checkpointed step
# ---------------------------------------------------------------------------

def row_exchange_enabled() -> bool:
    """DM_NO_ROW_EXCHANGE=1 restores the two out-of-place index_copy lines
    of runtime.step."""
    return os.environ.get("DM_NO_ROW_EXCHANGE", "0") != "1"


def _native_rows(ops, *ts):
    return hasattr(ops, "r_move_rows") and all(
        t.is_cuda and t.dtype == torch.float32 for t in ts)


def _move_rows(ops, src, si, dst, di, add=False):
    """dst[di] (=|+=) src[si] by rows, in place over a dst the caller owns:
    one kernel where the backend has r_move_rows, else torch index ops.
    di is unique, so the add rounds once per element either way."""
    if _native_rows(ops, src, dst):
        ops.r_move_rows(src.contiguous(), si, dst, di, add)
    elif add:
        dst.index_add_(0, di, src.index_select(0, si))
    else:
        dst.index_copy_(0, di, src.index_select(0, si))


def _zero_rows(ops, dst, di):
    if _native_rows(ops, dst):
        ops.r_zero_rows(dst, di)
    else:
        dst.index_fill_(0, di, 0)


def _own(g):
    """A contiguous copy of an incoming gradient, which is never written."""
    return g.clone(memory_format=torch.contiguous_format)


class _EdgeToBondFn(torch.autograd.Function):
    """(e, n_prev) -> (e, n_c): n_c = n_prev.index_copy(map_ude, e[map_de]).

    e is handed back as is and marked dirty, although nothing is written to
    it: its history then runs block -> this -> bond_to_edge -> next block as
    ONE consumer chain, and the backward receives the gradient of e and the
    gradient of n_c together.  Left as two consumers of e (this gather and
    the next user), autograd sums two dense [E,d] gradients of which one is
    zero outside the 4M mapped rows, after building that one with a zero
    fill, a sort and an index_put.  Here: one copy of G_e and one row kernel.
    """

    @staticmethod
    def forward(ctx, e, n_prev, pd, ops):
        B, M = n_prev.shape[0], len(pd.map_ude)
        # map_ude is unique: with B == M it names every row
        n_c = torch.empty_like(n_prev, memory_format=torch.contiguous_format) \
            if B == M else _own(n_prev)
        _move_rows(ops, e, pd.map_de, n_c, pd.map_ude)
        ctx.mark_dirty(e)
        ctx.set_materialize_grads(False)
        ctx.pd, ctx.ops, ctx.e_shape = pd, ops, e.shape
        return e, n_c

    @staticmethod
    def backward(ctx, G_e, G_nc):
        pd, ops = ctx.pd, ctx.ops
        if G_nc is None:
            return G_e, None, None, None
        ge = gn = None
        if ctx.needs_input_grad[0]:
            ge = _own(G_e) if G_e is not None else G_nc.new_zeros(ctx.e_shape)
            _move_rows(ops, G_nc, pd.map_ude, ge, pd.map_de, add=True)
        if ctx.needs_input_grad[1]:
            gn = _own(G_nc)
            _zero_rows(ops, gn, pd.map_ude)
        return ge, gn, None, None


class _BondToEdgeFn(torch.autograd.Function):
    """(e, n2) -> e with e[map_de] = n2[map_ude], written IN PLACE over e
    (the out-of-place index_copy clones all of e to change 4M rows)."""

    @staticmethod
    def forward(ctx, e, n2, pd, ops):
        _move_rows(ops, n2, pd.map_ude, e, pd.map_de)
        ctx.mark_dirty(e)
        ctx.pd, ctx.ops, ctx.n_shape = pd, ops, n2.shape
        return e

    @staticmethod
    def backward(ctx, go):
        pd, ops = ctx.pd, ctx.ops
        ge = gn2 = None
        if ctx.needs_input_grad[1]:
            full = ctx.n_shape[0] == len(pd.map_ude)
            gn2 = go.new_empty(ctx.n_shape) if full \
                else go.new_zeros(ctx.n_shape)
            _move_rows(ops, go, pd.map_de, gn2, pd.map_ude)
        if ctx.needs_input_grad[0]:
            ge = _own(go)
            _zero_rows(ops, ge, pd.map_de)
        return ge, gn2, None, None


def edge_to_bond(e, n_prev, pd, ops):
    """(e, n_c) with n_c = n_prev.index_copy(0, pd.map_ude, e[pd.map_de]);
    go on with the returned e (same storage) so that e keeps one consumer.
    Only where no saved tensor aliases e: the checkpointed steps."""
    return _EdgeToBondFn.apply(e, n_prev, pd, ops)


def bond_to_edge(e, n2, pd, ops):
    """e.index_copy(0, pd.map_de, n2[pd.map_ude]) written in place over e."""
    return _BondToEdgeFn.apply(e, n2, pd, ops)


def atom_block_available(ops, pe, d, dtype) -> bool:
    """Self-recomputing block policy for checkpointed steps: fp32, d = 64,
    frozen weights, recording mode, a backend with the raw fused first
    layer and its reverse.  DM_NO_ATOM_BLOCK=1 keeps torch.utils.checkpoint
    around the op-by-op block; DM_FUSED_CONV=1 and DM_NO_FUSED_MLP=1 keep
    their own paths."""
    return (os.environ.get("DM_NO_ATOM_BLOCK", "0") != "1"
            and os.environ.get("DM_FUSED_CONV", "0") != "1"
            and os.environ.get("DM_NO_FUSED_MLP", "0") != "1"
            and d == 64 and dtype == torch.float32
            and hasattr(ops, "r_edge_mlp3") and hasattr(ops, "r_edge_mlp_bwd")
            and hasattr(ops, "edge_mlp3_act")
            and not pe[0].requires_grad
            and torch.is_grad_enabled())


def _lean_bond(ops, pd, n, a, v, w3, pb, d):
    wcg, bcg, w2, b2, fusedT = pb
    w1, wn2, wv = wcg[:, :d], wcg[:, d:2 * d], wcg[:, 3 * d:]
    wl = ops.gather(w3, pd.l_src, csr=pd.line_src_csr)
    if (_fused_full(ops, d, "gated_mlp4_act")
            and not _records(n, a, v, wl)):
        msg = ops.gated_mlp4_act(a, fusedT, bcg, n @ w1.t(), n @ wn2.t(),
                                 v @ wv.t(), pd, w2, b2, wl, None)
        return ops.scatter_lines(msg, pd, base=n)
    if d == 64 and hasattr(ops, "edge_mlp4_act"):
        h = ops.edge_mlp4_act(a, fusedT, bcg, n @ w1.t(), n @ wn2.t(),
                              v @ wv.t(), pd)
    else:
        h = ops.gather_add4_act(n @ w1.t(), n @ wn2.t(),
                                torch.addmm(bcg, a, wcg[:, 2 * d:3 * d].t()),
                                v @ wv.t(), pd)
    msg = _mlp_tail_act(ops, h, w2, b2, wl, None, d)
    return ops.scatter_lines(msg, pd, base=n)


def _lean_angle(ops, pd, n, a, v, pa, d):
    wcg, bcg, w2, b2, fusedT = pa
    w1, wn2, wv = wcg[:, :d], wcg[:, d:2 * d], wcg[:, 3 * d:]
    if (_fused_full(ops, d, "gated_mlp4_act") and not _records(n, a, v)):
        return ops.gated_mlp4_act(a, fusedT, bcg, n @ w1.t(), n @ wn2.t(),
                                  v @ wv.t(), pd, w2, b2, None, a)
    if d == 64 and hasattr(ops, "edge_mlp4_act"):
        h = ops.edge_mlp4_act(a, fusedT, bcg, n @ w1.t(), n @ wn2.t(),
                              v @ wv.t(), pd)
    else:
        h = ops.gather_add4_act(n @ w1.t(), n @ wn2.t(),
                                torch.addmm(bcg, a, wcg[:, 2 * d:3 * d].t()),
                                v @ wv.t(), pd)
    return _mlp_tail_act(ops, h, w2, b2, None, a, d)


def _edge_to_bond(pd, n, e):
    return n.index_copy(0, pd.map_ude, e[pd.map_de])


def _keep_packs(pe, pn):
    """The atom packs _WholeGraphFn's keep mode hands to atom_fwd /
    atom_bwd: with fusedT, so the fused first layer and its reverse kernels
    run; DM_NO_ATOM_BLOCK=1 restores the 4-packs (rocBLAS first layer), as
    it restores the checkpointed steps' op-by-op blocks."""
    if os.environ.get("DM_NO_ATOM_BLOCK", "0") == "1":
        return pe[:4], pn[:4]
    return pe, pn


class _WholeGraphFn(torch.autograd.Function):
    """ALL message-passing blocks of one step — (n_blocks-1) x [atom conv;
    edge_to_bond; bond conv; bond_to_edge; angle conv] + the final atom
    conv (reference chgnet.py:296-368 + 400-419) — as ONE autograd
    Function with a fully hand-sequenced reverse pass.

    Single-partition only (halos are autograd boundaries).  The
    cross-conv gradient chains that autograd accumulates with separate
    elementwise add passes (the residual ~12.6 ms/step at li100k,
    profiles/r38) land as addmm_/add_ accumulations into persistent
    buffers; shared-weight grads (w_bb/w_ab/w_3b, consumed by every
    block) accumulate in place across blocks.

    recompute=True re-runs each block's forward inside backward (from
    saved block INPUTS) via the lean no-z forward — the hand-rolled
    equivalent of activation checkpointing, needed at si1m where saved
    z/cg would exceed HBM.

    Returns (v_final, v_mid); v_mid (the pre-final-block node features
    feeding sitewise_readout, chgnet.py:391-398) is non-differentiable.
    """

    @staticmethod
    def forward(ctx, e0, a0, wbb, wab, w3, v0, pd, ops, packs, d, nb,
                use_bg, recompute):
        keep = not recompute
        block_inputs, saves = [], []
        v, e, a = v0, e0, a0
        n = v0.new_empty(pd.n_bonds, d).index_copy_(
            0, pd.map_ude, e0[pd.map_de]) if use_bg else None
        for i in range(nb - 1):
            block_inputs.append((v, e, n, a))
            pe, pn = packs["atom"][i]
            if keep:
                v, e, sv_at = atom_fwd(ops, pd, v, e, wbb, wab,
                                       *_keep_packs(pe, pn), d)
            else:
                v, e = _lean_atom(ops, pd, v, e, wbb, wab, pe, pn, d)
                sv_at = None
            sv = {"atom": sv_at}
            if use_bg:
                n_c = _edge_to_bond(pd, n, e)
                if keep:
                    n, sv_b = bond_fwd(ops, pd, n_c, a, v, w3,
                                       packs["bond"][i][:4], d)
                    sv["bond"] = sv_b
                else:
                    n = _lean_bond(ops, pd, n_c, a, v, w3,
                                   packs["bond"][i], d)
                e = e.index_copy(0, pd.map_de, n[pd.map_ude])
                if i < nb - 2:
                    if keep:
                        a, sv_a = angle_fwd(ops, pd, n, a, v,
                                            packs["angle"][i][:4], d)
                        sv["angle"] = sv_a
                    else:
                        a = _lean_angle(ops, pd, n, a, v,
                                        packs["angle"][i], d)
            saves.append(sv)
        v_mid, e_mid = v, e
        pe, pn = packs["atom"][nb - 1]
        if keep:
            v2, _, sv_f = atom_fwd(ops, pd, v, e, wbb, wab,
                                   *_keep_packs(pe, pn), d)
        else:
            v2, _ = _lean_atom(ops, pd, v_mid, e_mid, wbb, wab, pe, pn, d)
            sv_f = None
        ctx.block_inputs = block_inputs
        ctx.saves = saves
        ctx.sv_f = sv_f
        ctx.final_in = (v_mid, e_mid)
        ctx.meta = (pd, ops, packs, d, nb, use_bg, recompute)
        ctx.w = (wbb, wab, w3)
        ctx.mark_non_differentiable(v_mid)
        ctx.set_materialize_grads(False)
        return v2, v_mid

    @staticmethod
    def backward(ctx, go_v2, _go_vmid):
        pd, ops, packs, d, nb, use_bg, recompute = ctx.meta
        wbb, wab, w3 = ctx.w
        with torch.no_grad():
            gwbb = torch.zeros_like(wbb)
            gwab = torch.zeros_like(wab)
            gw3 = torch.zeros_like(w3) if use_bg else None

            # final atom conv reverse (e output unused -> go_e2 None)
            v_mid, e_mid = ctx.final_in
            pe, pn = packs["atom"][nb - 1]
            sv_f = ctx.sv_f
            if sv_f is not None:
                gv, ge, _, _ = atom_bwd(ops, pd, sv_f,
                                        *_keep_packs(pe, pn), d,
                                        wbb, wab, go_v2, None,
                                        acc_wbb=gwbb, acc_wab=gwab)
                ctx.sv_f = None
            else:
                # streamed recompute: at most one MLP's [E,2d] saves live
                gv, ge = atom_bwd_recompute(ops, pd, v_mid, e_mid, wbb,
                                            wab, pe, pn, d, go_v2, None,
                                            gwbb, gwab)
            ctx.final_in = None
            ga = None
            gn = None

            for i in reversed(range(nb - 1)):
                v_in, e_in, n_in, a_in = ctx.block_inputs[i]
                sv = ctx.saves[i]
                pe, pn = packs["atom"][i]
                if recompute:
                    # re-run the pieces of this block's forward the
                    # reverse needs, lean where possible
                    if use_bg:
                        v_a, e_a = _lean_atom(ops, pd, v_in, e_in, wbb,
                                              wab, pe, pn, d)
                        n_c = _edge_to_bond(pd, n_in, e_a)
                        del e_a
                    sv_at = sv_b = sv_a = None
                else:
                    sv_at = sv["atom"]
                    sv_b = sv.get("bond")
                    sv_a = sv.get("angle")
                ctx.block_inputs[i] = None
                ctx.saves[i] = None

                if use_bg:
                    if ga is None:
                        ga = torch.zeros(pd.n_lines if hasattr(
                            pd, "n_lines") else len(pd.l_src), d,
                            dtype=gv.dtype, device=gv.device)
                    gn_b = gn if gn is not None else \
                        torch.zeros(pd.n_bonds, d, dtype=gv.dtype,
                                    device=gv.device)
                    if i < nb - 2:
                        if sv_a is None:
                            n_b = _lean_bond(ops, pd, n_c, a_in, v_a, w3,
                                             packs["bond"][i], d)
                            _, sv_a = angle_fwd(ops, pd, n_b, a_in, v_a,
                                                packs["angle"][i][:4], d)
                            del n_b
                        # angle reverse: n/v contributions accumulate,
                        # da replaces ga (includes its pass-through)
                        _, ga_new, _ = angle_bwd(
                            ops, pd, sv_a, packs["angle"][i][:4], d, ga,
                            acc_n=gn_b, acc_v=gv)
                        ga = ga_new
                        sv_a = None
                    # bond_to_edge reverse: e_b = e_a.index_copy(map_de,
                    # n_b[map_ude])
                    gn_b.index_add_(0, pd.map_ude, ge[pd.map_de])
                    ge = ge.index_fill(0, pd.map_de, 0)
                    # bond conv reverse (a/v/w3 contributions accumulate)
                    if sv_b is None:
                        _, sv_b = bond_fwd(ops, pd, n_c, a_in, v_a, w3,
                                           packs["bond"][i][:4], d)
                        del n_c
                    gn_c, _, _, _ = bond_bwd(ops, pd, sv_b,
                                             packs["bond"][i][:4], d, gn_b,
                                             acc_w3=gw3, acc_a=ga,
                                             acc_v=gv)
                    sv_b = None
                    del gn_b
                    # edge_to_bond reverse: n_c = n_in.index_copy(map_ude,
                    # e_a[map_de])
                    ge.index_add_(0, pd.map_de, gn_c[pd.map_ude])
                    gn = gn_c.index_fill(0, pd.map_ude, 0) \
                        if pd.n_bonds != len(pd.map_ude) else None
                    del gn_c

                if sv_at is not None:
                    gv, ge, _, _ = atom_bwd(ops, pd, sv_at,
                                            *_keep_packs(pe, pn),
                                            d, wbb, wab, gv, ge,
                                            acc_wbb=gwbb, acc_wab=gwab)
                else:
                    if use_bg:
                        del v_a
                    gv, ge = atom_bwd_recompute(ops, pd, v_in, e_in, wbb,
                                                wab, pe, pn, d, gv, ge,
                                                gwbb, gwab)

            # initial n0 = empty.index_copy(map_ude, e0[map_de])
            if use_bg and gn is not None:
                ge.index_add_(0, pd.map_de, gn[pd.map_ude])
        return (ge, ga, gwbb, gwab, gw3, gv, None, None, None, None,
                None, None, None)


def whole_graph_available(ops, mlp_pack) -> bool:
    """Whole-graph sequenced-reverse policy: single partition, frozen
    weights, raw-primitive backend, recording mode.  Default follows the
    measured A/B (DM_WHOLE_GRAPH=1/0 overrides)."""
    default = "1"          # keep-mode measured win (runtime gates ckpt mode)
    return (os.environ.get("DM_WHOLE_GRAPH", default) == "1"
            and hasattr(ops, "r_gather_add3")
            and not mlp_pack[0].requires_grad
            and torch.is_grad_enabled())


def _lean_edge_update(ops, pd, v, e, wbb, pe, d):
    """e2 only (no z/cg kept) — first half of the atom conv."""
    wcg1, bcg1, w21, b21, fusedT1 = pe
    ws1, wd1 = wcg1[:, :d], wcg1[:, d:2 * d]
    if d == 64 and hasattr(ops, "edge_mlp3_act"):
        h1 = ops.edge_mlp3_act(e, fusedT1, bcg1, v @ ws1.t(), v @ wd1.t(),
                               pd)
    else:
        h1 = ops.gather_add3_act(v @ ws1.t(), v @ wd1.t(),
                                 torch.addmm(bcg1, e, wcg1[:, 2 * d:].t()),
                                 pd)
    return _mlp_tail_act(ops, h1, w21, b21, wbb, e, d)


def atom_bwd_recompute(ops, pd, v_in, e_in, wbb, wab, pe, pn, d,
                       go_v2, go_e2, acc_wbb, acc_wab):
    """Streamed recompute + reverse of one atom conv from its INPUTS:
    the node MLP's z/cg are recomputed, reversed and FREED before the
    edge MLP's are materialized, so at most one MLP's [E,2d] saves are
    live — the memory shape that fits si1m's 46M edges (a single
    all-at-once recompute OOMs at ~94 GB of z/cg)."""
    ws1, wd1, we1, bcg1, w21, _ = _unpack_edge(pe[:4], d)
    ws2, wd2, we2, bcg2, w22, _ = _unpack_edge(pn[:4], d)
    go_v2 = go_v2.contiguous() if go_v2 is not None else None
    go_e2 = go_e2.contiguous() if go_e2 is not None else None

    if go_v2 is not None:
        e2 = _lean_edge_update(ops, pd, v_in, e_in, wbb, pe, d)
        z2, h2 = ops.r_gather_add3(v_in @ ws2.t(), v_in @ wd2.t(),
                                   torch.addmm(bcg2, e2, we2.t()), pd)
        del e2
        # cg only: the reverse below needs no out, so the GEMM alone
        # (4 [E,d] units of traffic) is less work than the fused tail (5+)
        cg2 = _second_fwd(h2, w22, pn[3], d)
        del h2
        dmsg = ops.r_gather_dst(go_v2, pd)
        dz2, dwab = _mlp_tail_bwd(ops, dmsg, cg2, wab, z2, w22, d)
        del dmsg, cg2, z2
        ge2 = (torch.addmm(go_e2, dz2, we2) if go_e2 is not None
               else dz2 @ we2)
        acc_wab.add_(dwab)
        del dwab
    else:
        dz2 = None
        ge2 = go_e2

    z1, h1 = ops.r_gather_add3(v_in @ ws1.t(), v_in @ wd1.t(),
                               torch.addmm(bcg1, e_in, we1.t()), pd)
    cg1 = _second_fwd(h1, w21, pe[3], d)
    del h1
    dz1, dwbb = _mlp_tail_bwd(ops, ge2, cg1, wbb, z1, w21, d)
    del cg1, z1
    ge = torch.addmm(ge2, dz1, we1)
    del ge2
    gv = torch.addmm(go_v2, ops.r_seg_src(dz1, pd), ws1) \
        if go_v2 is not None else ops.r_seg_src(dz1, pd) @ ws1
    gv.addmm_(ops.r_seg_dst(dz1, pd), wd1)
    del dz1
    if dz2 is not None:
        gv.addmm_(ops.r_seg_src(dz2, pd), ws2)
        gv.addmm_(ops.r_seg_dst(dz2, pd), wd2)
        del dz2
    acc_wbb.add_(dwbb)
    del dwbb
    return gv, ge
