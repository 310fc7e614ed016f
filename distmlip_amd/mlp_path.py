"""Which kernel path a CHGNet gated MLP, conv block or step takes.

Every A/B switch of the CHGNet path is listed in SWITCHES and read here, at
call time (tests flip them between two calls of one process).  conv.py,
chgnet.py, ops.py and runtime.py ask the predicates below and neither read
the environment nor probe the backend themselves.

A predicate is "the backend has the primitive, d == 64, and the switches
allow it".  Capability is asked of the backend object (hasattr), so a
backend without the optional primitives of ops_base (the fp64 reference
backend of the tests) takes the unfused forms of conv.py and chgnet.py.
What one switch turns off beyond its own kernel follows from the predicates
that call each other:

    whole-MLP kernel   needs the fused first layer and the fused tail forward
    factored weights   need both fused tails
    atom block         needs the fused first layer and no DM_FUSED_CONV
    lazy exchange      needs the row exchange, the atom block and the fused
                       first-layer reverse
    line block         needs the atom block, the three-gather fused first
                       layer, both fused tails with w_idx (the reverse one
                       with go_idx too), and the fused first-layer reverse
"""
from __future__ import annotations

import os

# name -> (value when unset, what "1" does)
SWITCHES = {
    "DM_NO_FUSED_MLP": ("0", "first layers run as rocBLAS addmm + the "
                        "gather-add kernel instead of the fused edge-MLP "
                        "kernel"),
    "DM_FUSED_MLP": ("1", "accepted and ignored: the fused first layer is "
                     "the default"),
    "DM_NO_FUSED_MLP_BWD": ("0", "reverse tails run as combine reverse, two "
                            "GEMMs and the silu reverse instead of one "
                            "kernel"),
    "DM_NO_FUSED_MLP_FWD": ("0", "forward tails run as baddbmm + the combine "
                            "kernel instead of one kernel"),
    "DM_NO_FUSED_MLP1_BWD": ("0", "the first layer's reverse runs as rocBLAS "
                             "GEMM / addmm instead of the kernel with the "
                             "gradient sum in its epilogue"),
    "DM_NO_FUSED_MLP_FULL": ("0", "a whole MLP runs as the first-layer + "
                             "tail kernel pair instead of one kernel"),
    "DM_NO_FACTORED_W": ("0", "blocks build the dense [E,d] message weights "
                         "(bexp @ W.t() by rocBLAS) instead of handing the "
                         "factors to the tail kernels"),
    "DM_NO_ATOM_BLOCK": ("0", "checkpointed steps keep torch.utils.checkpoint "
                         "around the op-by-op atom block, and the whole-graph "
                         "keep mode its rocBLAS first layers"),
    "DM_NO_FINAL_KEEP": ("0", "the final atom block of a checkpointed step "
                         "recomputes its saves like the others"),
    "DM_NO_ROW_EXCHANGE": ("0", "checkpointed steps move edge/bond rows with "
                           "the two out-of-place index_copy lines"),
    "DM_FUSED_CONV": ("0", "recording steps run each conv as one Function "
                      "with the hand-sequenced reverse (measured ~1% slower "
                      "than op-by-op, so opt-in)"),
    "DM_WHOLE_GRAPH": ("1", "single-partition steps run all blocks as one "
                       "Function with a hand-sequenced reverse; 0 restores "
                       "the op-by-op path"),
    "DM_WHOLE_GRAPH_CKPT": ("0", "checkpointed steps take the whole-graph "
                            "Function too, in its streamed-recompute mode "
                            "(measured slower at si1m, so opt-in)"),
}


def is_set(name: str) -> bool:
    """Whether switch `name` reads "1" in the environment right now."""
    return os.environ.get(name, SWITCHES[name][0]) == "1"


def _can(ops, d, prim, *off):
    return (d == 64 and hasattr(ops, prim)
            and not any(is_set(s) for s in off))


# -- one gated MLP ----------------------------------------------------------

def fused_first(ops, d, prim="edge_mlp3_act") -> bool:
    """First layer with its per-edge GEMM inside the gather kernel: `prim` is
    edge_mlp3_act / edge_mlp4_act (autograd forms) or r_edge_mlp3 (raw)."""
    return _can(ops, d, prim, "DM_NO_FUSED_MLP")


def fused_first_bwd(ops, d) -> bool:
    """Reverse of the fused first layer as r_edge_mlp_bwd."""
    return _can(ops, d, "r_edge_mlp_bwd", "DM_NO_FUSED_MLP1_BWD")


def fused_tail_fwd(ops, d, prim="r_mlp_tail_fwd") -> bool:
    """Second layer + combine in one kernel: r_mlp_tail_fwd (keeps cg) or
    mlp_tail_act (out only)."""
    return _can(ops, d, prim, "DM_NO_FUSED_MLP_FWD")


def fused_tail_bwd(ops, d, prim="r_mlp_tail_bwd") -> bool:
    """From the tail's output gradient to dz in one kernel: r_mlp_tail_bwd
    (raw) or mlp_tail (the autograd node whose backward it is)."""
    return _can(ops, d, prim, "DM_NO_FUSED_MLP_BWD")


def indexed_tail_bwd(ops, d) -> bool:
    """r_mlp_tail_bwd reading its gradient through an index (go_idx)."""
    return fused_tail_bwd(ops, d) and getattr(ops, "tail_bwd_indexed", False)


def _whole_mlp(ops, d, prim, first, tail) -> bool:
    return (_can(ops, d, prim, "DM_NO_FUSED_MLP_FULL")
            and fused_first(ops, d, first) and fused_tail_fwd(ops, d, tail))


def whole_mlp_keep(ops, d) -> bool:
    """A two-gather MLP as the one kernel r_gated_mlp3 (keeps z and cg)."""
    return _whole_mlp(ops, d, "r_gated_mlp3", "r_edge_mlp3", "r_mlp_tail_fwd")


def whole_mlp_act(ops, d) -> bool:
    """A three-gather MLP as the one kernel gated_mlp4_act (out only)."""
    return _whole_mlp(ops, d, "gated_mlp4_act", "edge_mlp4_act",
                      "mlp_tail_act")


def whole_mlp4_keep(ops, d) -> bool:
    """A three-gather MLP as the one kernel r_gated_mlp4 (keeps z and cg)."""
    return _whole_mlp(ops, d, "r_gated_mlp4", "edge_mlp4_act",
                      "r_mlp_tail_fwd")


def factored_w(ops, d) -> bool:
    """The tail kernels take a block's message weights as factors
    (ops.RadialW) and the dense [E,d] arrays are never built."""
    return (getattr(ops, "factored_w", False)
            and not is_set("DM_NO_FACTORED_W")
            and fused_tail_fwd(ops, d) and fused_tail_bwd(ops, d))


# DM_NO_FUSED_SEG=1: atom_bwd takes the dst segment sums of dz from
# r_seg_dst launches instead of the reverse tails' epilogues.  Read at call
# time like SWITCHES; it turns no other predicate off.
NO_FUSED_SEG = "DM_NO_FUSED_SEG"


def fused_seg(ops, d) -> bool:
    """r_mlp_tail_bwd also returns r_seg_dst(dz) for a factored w that
    carries the graph (RadialW.with_seg)."""
    return (getattr(ops, "tail_bwd_seg", False) and factored_w(ops, d)
            and os.environ.get(NO_FUSED_SEG, "0") != "1")


def line_seg(ops, d) -> bool:
    """r_mlp_tail_bwd also returns the l_dst segment sums of dz for a dense w
    with seg= (ops.LineSeg)."""
    return (getattr(ops, "tail_bwd_seg", False) and getattr(ops, "w_idx", False)
            and fused_tail_bwd(ops, d)
            and os.environ.get(NO_FUSED_SEG, "0") != "1")


# DM_NO_FUSED_SRC_SEG=1: the src segment sums of dz come from r_seg_src /
# r_seg_lsrc launches instead of the first layer's reverse kernel.  Read at
# call time like SWITCHES; it turns no other predicate off.
NO_FUSED_SRC_SEG = "DM_NO_FUSED_SRC_SEG"


def fused_src_seg(ops, d) -> bool:
    """The first layer's reverse runs as r_edge_mlp_bwd_src, which walks the
    rows in src order and also returns the src segment sums of dz."""
    return (_can(ops, d, "r_edge_mlp_bwd_src") and fused_first_bwd(ops, d)
            and os.environ.get(NO_FUSED_SRC_SEG, "0") != "1")


# -- conv blocks and whole steps ---------------------------------------------

def fused_keep_packs() -> bool:
    """The whole-graph keep mode hands atom_fwd / atom_bwd the 5-packs
    (fused first layer and reverse) rather than the 4-packs."""
    return not is_set("DM_NO_ATOM_BLOCK")


def atom_block(ops, d) -> bool:
    """Checkpointed steps run an atom block as the self-recomputing
    conv._AtomBlockFn: the raw fused first layer, its reverse kernel and the
    no-z autograd form."""
    return (fused_keep_packs() and not is_set("DM_FUSED_CONV")
            and fused_first(ops, d, "r_edge_mlp3")
            and hasattr(ops, "r_edge_mlp_bwd")
            and hasattr(ops, "edge_mlp3_act"))


# DM_NO_LINE_BLOCK=1: checkpointed steps keep torch.utils.checkpoint around
# the op-by-op bond and angle blocks.  Read at call time like SWITCHES; it
# turns no other predicate off.
NO_LINE_BLOCK = "DM_NO_LINE_BLOCK"


def line_block(ops, d) -> bool:
    """Checkpointed steps run a bond or angle block as the self-recomputing
    conv._BondBlockFn / _AngleBlockFn: the three-gather MLP (one kernel where
    whole_mlp_act / whole_mlp4_keep allow, else the fused first layer + tail
    pair, the same bits) with w3 read through l_src (w_idx), and the reverse
    tail with go_idx, w_idx and the dense seg form."""
    return (atom_block(ops, d)
            and os.environ.get(NO_LINE_BLOCK, "0") != "1"
            and fused_first(ops, d, "r_edge_mlp4")
            and hasattr(ops, "edge_mlp4_act")
            and fused_tail_fwd(ops, d) and fused_tail_fwd(ops, d, "mlp_tail_act")
            and getattr(ops, "w_idx", False)
            and getattr(ops, "tail_bwd_seg", False)
            and indexed_tail_bwd(ops, d) and fused_first_bwd(ops, d))


def final_keep() -> bool:
    """The final atom block of a checkpointed step keeps its saves."""
    return not is_set("DM_NO_FINAL_KEEP")


def whole_graph_ckpt() -> bool:
    """Checkpointed steps may take the whole-graph Function."""
    return is_set("DM_WHOLE_GRAPH_CKPT")


def row_exchange() -> bool:
    """Checkpointed steps move edge/bond rows in place over e; the
    whole-graph Function does its own exchange."""
    return not is_set("DM_NO_ROW_EXCHANGE") and not whole_graph_ckpt()


# DM_NO_LAZY_EXCHANGE=1: the reverses of the edge/bond row exchange each copy
# the gradient of e and patch the exchanged rows, instead of leaving them to
# the consuming block's first-layer reverse kernel.  Read at call time like
# SWITCHES; it turns no other predicate off.
NO_LAZY_EXCHANGE = "DM_NO_LAZY_EXCHANGE"


def lazy_exchange(ops, d) -> bool:
    """The reverses of the row exchange copy nothing: the block that consumes
    the gradient of e reads the exchanged rows through r_edge_mlp_bwd's
    patch (conv.ExchangeHolder)."""
    return (os.environ.get(NO_LAZY_EXCHANGE, "0") != "1" and row_exchange()
            and getattr(ops, "edge_mlp_bwd_patch", False)
            and atom_block(ops, d) and fused_first_bwd(ops, d))


def native_rows(ops) -> bool:
    """The backend moves rows with one kernel (r_move_rows, r_zero_rows)."""
    return hasattr(ops, "r_move_rows")


def fused_conv(ops, prim="r_gather_add3") -> bool:
    """One hand-sequenced Function per conv: r_gather_add3 for the atom
    conv, r_gather_add4 for the bond conv."""
    return is_set("DM_FUSED_CONV") and hasattr(ops, prim)


def whole_graph(ops) -> bool:
    """All blocks of a step as conv._WholeGraphFn."""
    return is_set("DM_WHOLE_GRAPH") and hasattr(ops, "r_gather_add3")
