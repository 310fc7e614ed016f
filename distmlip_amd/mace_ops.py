"""Product-side MACE math (torch, GPU-ready, autograd-capable).

Computational primitives the MACE runtime composes per partition; the
oracle (oracle/mace_ref.py) restates the same operations with its own
einsums, so the two sides share only the so3 coupling constants — which
tests pin against sympy/scipy independently (tests/test_so3.py).

Feature layout: per-l blocks, dict {l: [N, C, 2l+1]} — hidden irreps
carry only l in (0,1); interaction targets carry l = 0..3.  All ops are
plain torch (rocBLAS GEMM / bmm under the hood); the scatter-add goes
through the ops backend's segmented-sum HIP kernel when on GPU.
"""
from __future__ import annotations

import math
from functools import lru_cache
from typing import Dict

import numpy as np
import torch

from distmlip_amd import so3
from distmlip_amd.mace_model import Interaction, MACECore, ProductBasis


def bessel_cutoff(r: torch.Tensor, r_max: float, n: int, p: int
                  ) -> torch.Tensor:
    """MACE radial embedding: BesselBasis (fixed freqs k*pi) times the
    polynomial cutoff envelope applied to the DISTANCE (standard MACE
    composition — unlike the CHGNet quirk which applies it to the RBF
    output)."""
    freqs = torch.arange(1, n + 1, dtype=r.dtype, device=r.device) * math.pi
    d = r.unsqueeze(-1)
    bessel = math.sqrt(2.0 / r_max) * torch.sin(freqs * d / r_max) / d
    u = r / r_max
    a = -(p + 1) * (p + 2) / 2.0
    b = float(p * (p + 2))
    c = -p * (p + 1) / 2.0
    env = 1.0 + a * u ** p + b * u ** (p + 1) + c * u ** (p + 2)
    env = torch.where(r <= r_max, env, torch.zeros_like(r))
    return bessel * env.unsqueeze(-1)


@lru_cache(maxsize=None)
def _cg_t(l1: int, l2: int, l3: int, dtype_str: str, device_str: str):
    return torch.tensor(so3.real_cg(l1, l2, l3),
                        dtype=getattr(torch, dtype_str),
                        device=torch.device(device_str))


def cg_t(l1, l2, l3, like: torch.Tensor) -> torch.Tensor:
    return _cg_t(l1, l2, l3, str(like.dtype).split(".")[-1],
                 str(like.device))


def _chan_mix(xl: torch.Tensor, w: torch.Tensor, s: float) -> torch.Tensor:
    """out[n,m,d] = s * sum_c w[m,c] x[n,c,d] as one tall GEMM
    ([N*d, C] x [C, C]) — never a batched tiny-tile einsum."""
    N, C, d = xl.shape
    y = xl.transpose(1, 2).reshape(N * d, C) @ w.t()
    return (y * s).view(N, d, C).transpose(1, 2)


def irreps_linear(lin, x: Dict[int, torch.Tensor], norm: bool = True
                  ) -> Dict[int, torch.Tensor]:
    """o3.Linear: per-l channel mix, 1/sqrt(C) path normalization."""
    out = {}
    for l in lin.ls:
        w = lin.w[str(l)]
        s = 1.0 / math.sqrt(w.shape[1]) if norm else 1.0
        out[l] = _chan_mix(x[l], w, s)
    return out


def skip_tp(inter: Interaction, x: Dict[int, torch.Tensor],
            species: torch.Tensor) -> Dict[int, torch.Tensor]:
    """FullyConnectedTensorProduct(x, one_hot(species)) restatement:
    per-element channel mix on the shared irreps, grouped by element to
    avoid materializing [N, C, C]."""
    out = {}
    C = next(iter(x.values())).shape[1]
    s = 1.0 / math.sqrt(C)
    for l in inter.skip_ls:
        W = inter.skip[str(l)]                       # [n_elem, C, C]
        xl = x[l]
        ol = torch.zeros_like(xl)
        for e in torch.unique(species):
            m = species == e
            ol = ol.index_put((m.nonzero(as_tuple=True)[0],),
                              _chan_mix(xl[m], W[e], s))
        out[l] = ol
    return out


def conv_tp_messages(inter: Interaction, gathered: Dict[int, torch.Tensor],
                     Y: torch.Tensor, tp_w: torch.Tensor
                     ) -> Dict[int, torch.Tensor]:
    """uvu tensor product per edge: for each path (l1,l2,l3),
    msg_l3 += w_path * CG(l1,l2,l3)(x_src[l1], Y[l2]).

    gathered: per-l SENDER node features per edge [E, C, d1] (caller
    gathers via the ops backend so the backward is a segmented
    reduction); Y: [E,16] SH of edge vectors; tp_w: [E, P, C] per-edge
    path weights (radial MLP output).  Returns per-l3 messages
    [E, C, d3].

    Formulation policy (measured, mace62k same box):
      * batch-E bmm of (C x d1)(d1 x d3) tiles: rocBLAS MT16x16 at ~1%
        of peak, 46.4 s/step — never used;
      * per-path broadcast multiply-accumulates (default): 1.67 s/step;
      * per-l1 z-outer + stacked-CG tall GEMM with chunked
        checkpointing (DM_MACE_TP=zouter): 2.46 s/step — the recompute
        and the [E,C,d1*16] z traffic outweigh the saved reduction
        kernels at these shapes; kept for experimentation and as the
        stepping stone to the fused HIP TP kernel.
    """
    import os
    if os.environ.get("DM_MACE_TP") == "zouter":
        return _conv_tp_zouter(inter, gathered, Y, tp_w)
    msgs: Dict[int, torch.Tensor] = {}
    for p, (l1, l2, l3) in enumerate(inter.paths):
        CG = cg_t(l1, l2, l3, Y)
        o2, d2 = so3.L_OFF[l2], so3.L_DIMS[l2]
        d1, d3 = so3.L_DIMS[l1], so3.L_DIMS[l3]
        yb = Y[:, o2:o2 + d2]
        # [E, d2] @ [d2, d1*d3] -> [E, d1, d3]
        yc = (yb @ CG.permute(1, 0, 2).reshape(d2, d1 * d3)).view(-1, d1, d3)
        xa = gathered[l1] * tp_w[:, p, :].unsqueeze(-1)    # [E, C, d1]
        m = xa[:, :, 0:1] * yc[:, 0, :].unsqueeze(1)
        for k1 in range(1, d1):
            m = m + xa[:, :, k1:k1 + 1] * yc[:, k1, :].unsqueeze(1)
        if l3 in msgs:
            msgs[l3] = msgs[l3] + m
        else:
            msgs[l3] = m
    return msgs


def _conv_tp_zouter(inter: Interaction, gathered: Dict[int, torch.Tensor],
                    Y: torch.Tensor, tp_w: torch.Tensor
                    ) -> Dict[int, torch.Tensor]:
    import os
    E = Y.shape[0]
    C = next(iter(gathered.values())).shape[1]
    by_l1: Dict[int, list] = {}
    for p, (l1, l2, l3) in enumerate(inter.paths):
        by_l1.setdefault(l1, []).append((p, l2, l3))
    l3s = sorted({l3 for (_, _, l3) in inter.paths})

    def tp_chunk(Y_c, w_c, *g_c):
        out = {}
        Ec = Y_c.shape[0]
        for gi, (l1, plist) in enumerate(by_l1.items()):
            d1 = so3.L_DIMS[l1]
            Cbig = _tp_cbig(l1, tuple(plist),
                            str(Y_c.dtype).split(".")[-1], str(Y_c.device))
            z = (g_c[gi].unsqueeze(-1) * Y_c.view(Ec, 1, 1, 16)
                 ).reshape(Ec, C, d1 * 16)
            u = z @ Cbig                              # [Ec, C, sum d3]
            col = 0
            for (p, l2, l3) in plist:
                d3 = so3.L_DIMS[l3]
                m = u[:, :, col:col + d3] * w_c[:, p, :].unsqueeze(-1)
                col += d3
                out[l3] = out[l3] + m if l3 in out else m
        return tuple(out[l3] for l3 in l3s)

    chunk = int(os.environ.get("DM_MACE_TP_CHUNK", 1_000_000))
    if E <= chunk:
        parts = [tp_chunk(Y, tp_w, *(gathered[l1] for l1 in by_l1))]
    else:
        # chunk edges; checkpoint each chunk so the z/u transients
        # (z is [E, C, 48] = 71 GB unchunked at 2.9M edges) are
        # recomputed per chunk during backward, never all live at once
        parts = []
        for e0 in range(0, E, chunk):
            e1 = min(e0 + chunk, E)
            args = (Y[e0:e1], tp_w[e0:e1],
                    *(gathered[l1][e0:e1] for l1 in by_l1))
            if torch.is_grad_enabled() and Y.requires_grad:
                parts.append(torch.utils.checkpoint.checkpoint(
                    tp_chunk, *args, use_reentrant=False))
            else:
                parts.append(tp_chunk(*args))
    return {l3: torch.cat([p[i] for p in parts], dim=0)
            for i, l3 in enumerate(l3s)}


@lru_cache(maxsize=None)
def _tp_cbig(l1: int, plist, dtype_str: str, device_str: str):
    """[d1*16, sum_p d3]: per path (l1,l2,l3), the CG block embedded at
    k2-rows of the l2 block, stacked column-wise in path order."""
    d1 = so3.L_DIMS[l1]
    cols = sum(so3.L_DIMS[l3] for (_, _, l3) in plist)
    Cbig = np.zeros((d1 * 16, cols))
    col = 0
    for (_, l2, l3) in plist:
        CG = so3.real_cg(l1, l2, l3)                  # [d1, d2, d3]
        o2, d2 = so3.L_OFF[l2], so3.L_DIMS[l2]
        d3 = so3.L_DIMS[l3]
        blk = np.zeros((d1, 16, d3))
        blk[:, o2:o2 + d2, :] = CG
        Cbig[:, col:col + d3] = blk.reshape(d1 * 16, d3)
        col += d3
    return torch.tensor(Cbig, dtype=getattr(torch, dtype_str),
                        device=torch.device(device_str))


@lru_cache(maxsize=None)
def _trees_M(nu: int, lo: int, dtype_str: str, device_str: str):
    trees, M = so3.symmetric_basis_trees(nu, lo)
    return trees, torch.tensor(M, dtype=getattr(torch, dtype_str),
                               device=torch.device(device_str))


@lru_cache(maxsize=None)
def _combo_groups(nu: int, lo: int, dtype_str: str, device_str: str):
    """Trees grouped by their (l1[,l2[,l3]]) slot signature, each group's
    coupling tensors stacked into ONE [d1*d2*d3, n_t*do] GEMM operand.
    Returns list of (combo, tree_indices, D) with D on device."""
    trees, _ = so3.symmetric_basis_trees(nu, lo)
    do = 2 * lo + 1
    dt = getattr(torch, dtype_str)
    dev = torch.device(device_str)
    groups = {}
    for t, tr in enumerate(trees):
        combo = tr if nu == 1 else (tr[:2] if nu == 2
                                    else (tr[0], tr[1], tr[3]))
        groups.setdefault(combo, []).append(t)
    out = []
    for combo, tidx in groups.items():
        Ds = []
        for t in tidx:
            tr = trees[t]
            if nu == 1:
                D = np.eye(2 * tr[0] + 1)
            elif nu == 2:
                D = so3.real_cg(tr[0], tr[1], lo).reshape(-1, do)
            else:
                l1, l2, L, l3 = tr
                C12 = so3.real_cg(l1, l2, L)
                C3 = so3.real_cg(L, l3, lo)
                D = np.einsum("abL,Lko->abko", C12, C3).reshape(-1, do)
            Ds.append(D)
        D = np.concatenate(Ds, axis=1)               # [prod d, n_t*do]
        out.append((combo, tidx,
                    torch.tensor(D, dtype=dt, device=dev)))
    return out


def symmetric_contract(prod: ProductBasis, x: Dict[int, torch.Tensor],
                       species: torch.Tensor, correlation: int
                       ) -> Dict[int, torch.Tensor]:
    """MACE SymmetricContraction: sum over nu=1..corr of per-element
    weighted symmetric couplings via the tree factorization
    (so3.symmetric_basis_trees) — no dense [16]^nu tensors at run time.

    Shape discipline: per slot-signature group, the couplings collapse to
    one tall-skinny GEMM [N*C, d1*d2*d3] x [d1*d2*d3, n_t*do] over the
    broadcast outer product of the slot blocks; per-tree weighting is a
    broadcast multiply.  (Per-tree einsums lowered to batch-N bmms of
    tiny tiles — the rocBLAS ~1%-of-peak shape, see
    conv_tp_messages.)"""
    like = next(iter(x.values()))
    if symc_hip_available(x, prod):
        return symmetric_contract_hip(prod, x, species, correlation)
    if symc_tree_available(x, prod):
        return symmetric_contract_tree(prod, x, species, correlation)
    N, C = like.shape[0], like.shape[1]
    dts, devs = str(like.dtype).split(".")[-1], str(like.device)
    out = {}
    for lo in prod.out_ls:
        do = 2 * lo + 1
        acc = like.new_zeros(N, C, do)
        for nu in range(1, correlation + 1):
            key = f"{lo}_{nu}"
            if key not in prod.weights:
                continue
            trees, M = _trees_M(nu, lo, dts, devs)
            T = len(trees)
            tvs: list = [None] * T
            for combo, tidx, D in _combo_groups(nu, lo, dts, devs):
                if nu == 1:
                    xx = x[combo[0]]
                elif nu == 2:
                    l1, l2 = combo
                    xx = (x[l1].unsqueeze(-1) * x[l2].unsqueeze(-2)
                          ).reshape(N, C, -1)
                else:
                    l1, l2, l3 = combo
                    xx = (x[l1].unsqueeze(-1) * x[l2].unsqueeze(-2)
                          ).reshape(N, C, -1)
                    xx = (xx.unsqueeze(-1) * x[l3].unsqueeze(-2)
                          ).reshape(N, C, -1)
                g = xx @ D                            # [N, C, n_t*do]
                for j, t in enumerate(tidx):
                    tvs[t] = g[:, :, j * do:(j + 1) * do]
            w = prod.weights[key]                    # [n_elem, P, C]
            wM = torch.einsum("epc,pt->etc", w, M)   # [n_elem, T, C]
            wMn = wM[species]                        # [N, T, C]
            tv = torch.stack(tvs, dim=-1)            # [N, C, do, T]
            acc = acc + (tv * wMn.permute(0, 2, 1).unsqueeze(2)).sum(-1)
        out[lo] = acc
    return out


def pad_missing(x: Dict[int, torch.Tensor], ls, like: torch.Tensor
                ) -> Dict[int, torch.Tensor]:
    N, C = like.shape[0], like.shape[1]
    out = dict(x)
    for l in ls:
        if l not in out:
            out[l] = like.new_zeros(N, C, 2 * l + 1)
    return out


# ---------------------------------------------------------------------------
# fused HIP tensor product (round 2): one wave per edge, CG nonzeros via
# the scalar cache, LDS accumulators — include/distmlip_hip.h
# ---------------------------------------------------------------------------

@lru_cache(maxsize=None)
def _tp_nz(paths_key, device_str):
    import numpy as np
    ents, coefs = [], []
    for p, (l1, l2, l3) in enumerate(paths_key):
        CG = so3.real_cg(l1, l2, l3)
        slot = 0 if l1 == 0 else 1
        for k1 in range(CG.shape[0]):
            for k2l in range(CG.shape[1]):
                for k3l in range(CG.shape[2]):
                    c = CG[k1, k2l, k3l]
                    if abs(c) > 1e-12:
                        ents.append([p, slot, k1,
                                     so3.L_OFF[l2] + k2l,
                                     so3.L_OFF[l3] + k3l])
                        coefs.append(c)
    dev = torch.device(device_str)
    nz = torch.tensor(np.asarray(ents, dtype=np.int32),
                      device=dev).contiguous().view(-1)
    nzc = torch.tensor(np.asarray(coefs, dtype=np.float32), device=dev)
    return nz, nzc


class _MaceTPFn(torch.autograd.Function):
    """Fused uvu TP: m [E,16,C] from x0 [E,C], x1 [E,C,d1b] (or None),
    Y [E,16], w [E,P,C] — forward and backward each ONE kernel."""

    @staticmethod
    def forward(ctx, x0, x1, Y, w, nz, nzc, P, d1b):
        from distmlip_amd.ops import _check, _fp, _ip, _stream, hip_lib
        E, C = x0.shape
        outs = [torch.empty(E, 2 * l3 + 1, C, dtype=x0.dtype,
                            device=x0.device) for l3 in range(4)]
        _check(hip_lib().dm_mace_tp_fwd_f32(
            _fp(x0), _fp(x1) if x1 is not None else None, _fp(Y), _fp(w),
            _ip(nz), _fp(nzc), nz.numel() // 5,
            _fp(outs[0]), _fp(outs[1]), _fp(outs[2]), _fp(outs[3]),
            E, C, P, max(d1b, 1), _stream()), "dm_mace_tp_fwd_f32")
        ctx.save_for_backward(x0, Y, w, nz, nzc)
        ctx.x1 = x1
        ctx.meta = (P, d1b)
        return tuple(outs)

    @staticmethod
    def backward(ctx, g0, g1, g2, g3):
        from distmlip_amd.ops import _check, _fp, _ip, _stream, hip_lib
        x0, Y, w, nz, nzc = ctx.saved_tensors
        x1 = ctx.x1
        P, d1b = ctx.meta
        E, C = x0.shape
        gs = [g.contiguous() for g in (g0, g1, g2, g3)]
        dx0 = torch.empty_like(x0)
        dx1 = torch.empty_like(x1) if x1 is not None else None
        dY = torch.empty_like(Y)
        dw = torch.empty_like(w)
        _check(hip_lib().dm_mace_tp_bwd_f32(
            _fp(gs[0]), _fp(gs[1]), _fp(gs[2]), _fp(gs[3]),
            _fp(x0), _fp(x1) if x1 is not None else None, _fp(Y),
            _fp(w), _ip(nz), _fp(nzc), nz.numel() // 5, _fp(dx0),
            _fp(dx1) if dx1 is not None else None, _fp(dY), _fp(dw),
            E, C, P, max(d1b, 1), _stream()), "dm_mace_tp_bwd_f32")
        return dx0, dx1, dY, dw, None, None, None, None


def conv_tp_hip_available(inter: Interaction, Y: torch.Tensor,
                          C: int) -> bool:
    import os
    return (os.environ.get("DM_MACE_TP", "hip") == "hip"
            and Y.is_cuda and C in (64, 128)
            and all(l1 in (0, 1) for (l1, _, _) in inter.paths))


def conv_tp_hip(inter: Interaction, x0: torch.Tensor,
                x1, Y: torch.Tensor, tp_w: torch.Tensor):
    """Returns (m0..m3): per-l3 messages [E, 2*l3+1, C] (contiguous rows
    for the scatter; note the l-major layout vs the torch path's
    [E, C, d3])."""
    paths_key = tuple(inter.paths)
    nz, nzc = _tp_nz(paths_key, str(Y.device))
    d1b = x1.shape[-1] if x1 is not None else 0
    P = len(inter.paths)
    return _MaceTPFn.apply(x0.contiguous(),
                           x1.contiguous() if x1 is not None else None,
                           Y.contiguous(), tp_w.contiguous(), nz, nzc,
                           P, d1b)


# ---------------------------------------------------------------------------
# fused HIP convolution: gather + uvu TP + dst sum in one kernel per pass,
# one wave per (node, 64-channel block) — csrc/mace_conv.hip.  No per-edge
# [E, *, C] array besides tp_w and its gradient.
# ---------------------------------------------------------------------------

def _conv_path_lists():
    from distmlip_amd.mace_model import tp_paths
    return (tuple(tp_paths((0,), 3)), tuple(tp_paths((0, 1), 3)))


@lru_cache(maxsize=None)
def _conv_K(paths_key, device_str):
    """K [T,16]: row t = (p, k1, k3) holds CG_p[k1, :, k3] at the columns
    of path p's l2 block, so yc[e,t] = sum_k2 K[t,k2] Y[e,k2]."""
    rows = []
    for (l1, l2, l3) in paths_key:
        CG = so3.real_cg(l1, l2, l3)
        o2, d2 = so3.L_OFF[l2], so3.L_DIMS[l2]
        for k1 in range(CG.shape[0]):
            for k3 in range(CG.shape[2]):
                row = np.zeros(16)
                row[o2:o2 + d2] = CG[k1, :, k3]
                rows.append(row)
    return torch.tensor(np.asarray(rows, dtype=np.float32),
                        device=torch.device(device_str))


class _MaceConvFn(torch.autograd.Function):
    """M [N,16,C] = sum over in-edges of the uvu product of xs[src] [N,R,C],
    Y [E,16], tp_w [E,P,C].  Forward one kernel over the dst CSR; backward
    one kernel per CSR (dw and dY over dst, dxs over the src permutation).
    Deterministic: no atomics."""

    @staticmethod
    def forward(ctx, xs, Y, tp_w, K, ls, src, dst, row_ptr, src_perm,
                src_row_ptr):
        from distmlip_amd.ops import _check, _chk_f32, _fp, _ip, _stream, \
            hip_lib
        _chk_f32(xs, Y, tp_w, K)
        N, _, C = xs.shape
        ctx.save_for_backward(xs, Y, tp_w)
        ctx.idx = (K, ls, src, dst, row_ptr, src_perm, src_row_ptr)
        if Y.shape[0] == 0:
            return xs.new_zeros(N, 16, C)
        M = torch.empty(N, 16, C, dtype=xs.dtype, device=xs.device)
        _check(hip_lib().dm_mace_conv_fwd_f32(
            _fp(xs), _fp(tp_w), _fp(Y), _fp(K), _ip(src), _ip(row_ptr),
            _fp(M), N, C, ls, _stream()), "dm_mace_conv_fwd_f32")
        return M

    @staticmethod
    def backward(ctx, G):
        from distmlip_amd.ops import _check, _fp, _ip, _stream, hip_lib
        xs, Y, tp_w = ctx.saved_tensors
        K, ls, src, dst, row_ptr, src_perm, src_row_ptr = ctx.idx
        N, _, C = xs.shape
        E = Y.shape[0]
        dxs = dY = dw = None
        if E == 0:
            return (torch.zeros_like(xs), torch.zeros_like(Y),
                    torch.zeros_like(tp_w)) + (None,) * 7
        G = G.contiguous()
        if ctx.needs_input_grad[0]:
            dxs = torch.empty_like(xs)
            _check(hip_lib().dm_mace_conv_bwd_node_f32(
                _fp(G), _fp(tp_w), _fp(Y), _fp(K), _ip(dst), _ip(src_perm),
                _ip(src_row_ptr), _fp(dxs), N, C, ls, _stream()),
                "dm_mace_conv_bwd_node_f32")
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw = torch.empty_like(tp_w)
            dYp = torch.empty(C // 64, E, 16, dtype=Y.dtype, device=Y.device)
            _check(hip_lib().dm_mace_conv_bwd_edge_f32(
                _fp(G), _fp(xs), _fp(tp_w), _fp(Y), _fp(K), _ip(src),
                _ip(row_ptr), _fp(dw), _fp(dYp), N, E, C, ls, _stream()),
                "dm_mace_conv_bwd_edge_f32")
            dY = dYp[0] if C == 64 else dYp.sum(0)
        return (dxs, dY, dw) + (None,) * 7


def conv_fused_available(inter: Interaction, Y: torch.Tensor, C: int, pd,
                         ops) -> bool:
    """DM_MACE_CONV=split pins the gather + conv_tp_hip + scatter path;
    =radial asks for conv_radial_hip and falls back to this one."""
    import os
    return (os.environ.get("DM_MACE_CONV", "fused") in ("fused", "radial")
            and os.environ.get("DM_MACE_TP", "hip") == "hip"
            and Y.is_cuda and Y.dtype == torch.float32
            and C % 64 == 0
            and tuple(inter.paths) in _conv_path_lists()
            and hasattr(pd, "src_perm")
            and not getattr(ops, "is_reference", False))


def conv_fused_hip(inter: Interaction, x_up: Dict[int, torch.Tensor],
                   Y: torch.Tensor, tp_w: torch.Tensor, pd
                   ) -> Dict[int, torch.Tensor]:
    """Summed messages {l3: [N, C, 2*l3+1]} straight from the node blocks
    x_up {l: [N, C, 2l+1]} (see _MaceConvFn); pd carries the int32 dst CSR
    and src permutation CSR of the graph builder."""
    paths_key = tuple(inter.paths)
    ls = _conv_path_lists().index(paths_key)
    K = _conv_K(paths_key, str(Y.device))
    xs = torch.cat([x_up[l].permute(0, 2, 1) for l in sorted(x_up)],
                   dim=1).contiguous()              # [N, R, C]
    assert xs.shape[1] == (1, 4)[ls], xs.shape
    M = _MaceConvFn.apply(xs, Y.contiguous(), tp_w.contiguous(), K, ls,
                          pd.src, pd.dst, pd.row_ptr, pd.src_perm,
                          pd.src_row_ptr)
    return {l3: M[:, so3.L_OFF[l3]:so3.L_OFF[l3] + so3.L_DIMS[l3], :]
            .permute(0, 2, 1).contiguous() for l3 in range(4)}


# ---------------------------------------------------------------------------
# the fused convolution with the radial MLP's last layer inside: tp_w =
# h @ Wr.T is formed per 16-edge tile on fp32 MFMA and never stored, and dw
# goes straight into dh.  Per-edge state: h [E,64], Y [E,16], their gradients.
# ---------------------------------------------------------------------------

RADIAL_H = 64


def _conv_wr_packed(inter: Interaction, C: int):
    """The last radial weight Wr [P*C, 64] in the MFMA operand orders of
    csrc/mace_conv.hip (Wa for w, Wb for dh; include/distmlip_hip.h);
    cached on the module while frozen."""
    Wr = inter.radial.layers[-1].weight
    key = (Wr.device, Wr._version)
    cached = getattr(inter, "_dm_wr_packed", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    P, CB = Wr.shape[0] // C, C // 64
    W = Wr.detach()
    Wa = W.view(P, CB, 4, 16, 4, 4, 4).permute(0, 1, 2, 5, 4, 3, 6)
    Wb = W.view(P, CB, 4, 4, 4, 4, 16).permute(0, 1, 5, 3, 2, 6, 4)
    packed = (Wa.contiguous(), Wb.contiguous())
    if not Wr.requires_grad:
        inter._dm_wr_packed = (key, packed)
    return packed


class _MaceConvRadialFn(torch.autograd.Function):
    """_MaceConvFn with tp_w = h @ Wr.T computed inside the kernels: M from
    xs [N,R,C], Y [E,16], h [E,64] and the packed Wr.  The backward gives
    dxs, dY and dh; Wr is frozen.  Deterministic: no atomics."""

    @staticmethod
    def forward(ctx, xs, Y, h, Wa, Wb, K, ls, src, dst, row_ptr, src_perm,
                src_row_ptr):
        from distmlip_amd.ops import _check, _chk_f32, _fp, _ip, _stream, \
            hip_lib
        _chk_f32(xs, Y, h, Wa, Wb, K)
        N, _, C = xs.shape
        ctx.save_for_backward(xs, Y, h)
        ctx.idx = (Wa, Wb, K, ls, src, dst, row_ptr, src_perm, src_row_ptr)
        if Y.shape[0] == 0:
            return xs.new_zeros(N, 16, C)
        M = torch.empty(N, 16, C, dtype=xs.dtype, device=xs.device)
        _check(hip_lib().dm_mace_conv_rad_fwd_f32(
            _fp(xs), _fp(h), _fp(Wa), _fp(Y), _fp(K), _ip(src), _ip(row_ptr),
            _fp(M), N, C, h.shape[1], ls, _stream()),
            "dm_mace_conv_rad_fwd_f32")
        return M

    @staticmethod
    def backward(ctx, G):
        from distmlip_amd.ops import _check, _fp, _ip, _stream, hip_lib
        xs, Y, h = ctx.saved_tensors
        Wa, Wb, K, ls, src, dst, row_ptr, src_perm, src_row_ptr = ctx.idx
        N, _, C = xs.shape
        E, H = h.shape
        dxs = dY = dh = None
        if E == 0:
            return (torch.zeros_like(xs), torch.zeros_like(Y),
                    torch.zeros_like(h)) + (None,) * 9
        G = G.contiguous()
        if ctx.needs_input_grad[0]:
            dxs = torch.empty_like(xs)
            _check(hip_lib().dm_mace_conv_rad_bwd_node_f32(
                _fp(G), _fp(h), _fp(Wa), _fp(Y), _fp(K), _ip(dst),
                _ip(src_perm), _ip(src_row_ptr), _fp(dxs), N, C, H, ls,
                _stream()), "dm_mace_conv_rad_bwd_node_f32")
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dhp = torch.empty(C // 64, E, H, dtype=h.dtype, device=h.device)
            dYp = torch.empty(C // 64, E, 16, dtype=Y.dtype, device=Y.device)
            _check(hip_lib().dm_mace_conv_rad_bwd_edge_f32(
                _fp(G), _fp(xs), _fp(h), _fp(Wa), _fp(Wb), _fp(Y), _fp(K),
                _ip(src), _ip(row_ptr), _fp(dhp), _fp(dYp), N, E, C, H, ls,
                _stream()), "dm_mace_conv_rad_bwd_edge_f32")
            dh = dhp[0] if C == 64 else dhp.sum(0)
            dY = dYp[0] if C == 64 else dYp.sum(0)
        return (dxs, dY, dh) + (None,) * 9


def conv_radial_available(inter: Interaction, Y: torch.Tensor, C: int, pd,
                          ops) -> bool:
    """DM_MACE_CONV=radial, where the fused convolution can run, the radial
    MLP's last layer is 64 wide and its weight frozen."""
    import os
    Wr = inter.radial.layers[-1].weight
    return (os.environ.get("DM_MACE_CONV", "fused") == "radial"
            and conv_fused_available(inter, Y, C, pd, ops)
            and Wr.shape[1] == RADIAL_H and not Wr.requires_grad)


def conv_radial_hip(inter: Interaction, x_up: Dict[int, torch.Tensor],
                    Y: torch.Tensor, h: torch.Tensor, pd
                    ) -> Dict[int, torch.Tensor]:
    """conv_fused_hip from h [E,64], the output of inter.radial.layers[:-1]
    with their SiLUs, in place of tp_w = h @ Wr.T (see _MaceConvRadialFn)."""
    paths_key = tuple(inter.paths)
    ls = _conv_path_lists().index(paths_key)
    K = _conv_K(paths_key, str(Y.device))
    xs = torch.cat([x_up[l].permute(0, 2, 1) for l in sorted(x_up)],
                   dim=1).contiguous()              # [N, R, C]
    assert xs.shape[1] == (1, 4)[ls], xs.shape
    Wa, Wb = _conv_wr_packed(inter, xs.shape[2])
    M = _MaceConvRadialFn.apply(xs, Y.contiguous(), h.contiguous(), Wa, Wb,
                                K, ls, pd.src, pd.dst, pd.row_ptr,
                                pd.src_perm, pd.src_row_ptr)
    return {l3: M[:, so3.L_OFF[l3]:so3.L_OFF[l3] + so3.L_DIMS[l3], :]
            .permute(0, 2, 1).contiguous() for l3 in range(4)}


def radial_hidden(inter: Interaction, edge_feats: torch.Tensor
                  ) -> torch.Tensor:
    """h [E,64]: the radial MLP up to its last layer, SiLUs included."""
    x = edge_feats
    for lin in inter.radial.layers[:-1]:
        x = torch.nn.functional.silu(lin(x))
    return x


# ---------------------------------------------------------------------------
# fused HIP symmetric contraction (round 2): one wave per node, polynomial
# entries via the scalar cache, x rows + accumulators in LDS.  Weights are
# FROZEN (inference engine) — backward produces dx only, so the
# availability check requires requires_grad=False weights.
# ---------------------------------------------------------------------------

@lru_cache(maxsize=None)
def _symc_nz(out_ls, correlation: int, device_str: str):
    import numpy as np
    ents, coefs = [], []
    wrow = 0
    o_off = 0
    meta = []                      # (lo, nu, n_trees) in wrow order
    for lo in out_ls:
        do = 2 * lo + 1
        for nu in range(1, correlation + 1):
            trees, _M = so3.symmetric_basis_trees(nu, lo)
            for tr in trees:
                if nu == 1:
                    (l,) = tr
                    for m in range(do):
                        ents.append([wrow, so3.L_OFF[l] + m, 16, 16,
                                     o_off + m])
                        coefs.append(1.0)
                elif nu == 2:
                    l1, l2 = tr
                    C = so3.real_cg(l1, l2, lo)
                    for a in range(C.shape[0]):
                        for b in range(C.shape[1]):
                            for oo in range(do):
                                c = C[a, b, oo]
                                if abs(c) > 1e-12:
                                    ents.append([wrow,
                                                 so3.L_OFF[l1] + a,
                                                 so3.L_OFF[l2] + b, 16,
                                                 o_off + oo])
                                    coefs.append(c)
                else:
                    l1, l2, L, l3 = tr
                    K = np.einsum("abL,Lko->abko",
                                  so3.real_cg(l1, l2, L),
                                  so3.real_cg(L, l3, lo))
                    nzs = np.argwhere(np.abs(K) > 1e-12)
                    for (a, b, k, oo) in nzs:
                        ents.append([wrow, so3.L_OFF[l1] + a,
                                     so3.L_OFF[l2] + b,
                                     so3.L_OFF[l3] + k, o_off + oo])
                        coefs.append(K[a, b, k, oo])
                wrow += 1
            meta.append((lo, nu, len(trees)))
        o_off += do
    dev = torch.device(device_str)
    # kernel reads sextuples; pad with a zero column
    arr = np.asarray(ents, dtype=np.int32)
    arr6 = np.zeros((len(ents), 6), dtype=np.int32)
    arr6[:, :5] = arr
    nz = torch.tensor(arr6, device=dev).contiguous().view(-1)
    nzc = torch.tensor(np.asarray(coefs, dtype=np.float32), device=dev)
    return nz, nzc, wrow, o_off, tuple(meta)


def _symc_wcat(prod: ProductBasis, correlation: int) -> torch.Tensor:
    """Per-element weight table [n_elem, T_total, C] in wrow order
    (tree-major within each (lo, nu)); cached on the module while
    frozen."""
    key = (next(iter(prod.weights.values())).device,
           tuple(p._version for p in prod.weights.values()))
    cached = getattr(prod, "_dm_wcat", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    dts = str(next(iter(prod.weights.values())).dtype).split(".")[-1]
    devs = str(next(iter(prod.weights.values())).device)
    cols = []
    for lo in prod.out_ls:
        for nu in range(1, correlation + 1):
            k = f"{lo}_{nu}"
            if k not in prod.weights:
                continue
            _, M = _trees_M(nu, lo, dts, devs)
            w = prod.weights[k]                      # [n_elem, P, C]
            cols.append(torch.einsum("epc,pt->etc", w, M))
    W = torch.cat(cols, dim=1).contiguous()
    if not any(p.requires_grad for p in prod.weights.values()):
        prod._dm_wcat = (key, W)
    return W


class _MaceSymcFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xs, elem, W, nz, nzc, S_out):
        from distmlip_amd.ops import _check, _fp, _ip, _stream, hip_lib
        N, _, C = xs.shape
        T = W.shape[1]
        out = torch.empty(N, S_out, C, dtype=xs.dtype, device=xs.device)
        _check(hip_lib().dm_mace_symc_fwd_f32(
            _fp(xs), _ip(elem), _fp(W), _ip(nz), _fp(nzc),
            nz.numel() // 6, _fp(out), N, C, T, S_out, _stream()),
            "dm_mace_symc_fwd_f32")
        ctx.save_for_backward(xs, elem, W, nz, nzc)
        ctx.S_out = S_out
        return out

    @staticmethod
    def backward(ctx, go):
        from distmlip_amd.ops import _check, _fp, _ip, _stream, hip_lib
        xs, elem, W, nz, nzc = ctx.saved_tensors
        N, _, C = xs.shape
        T = W.shape[1]
        dx = torch.empty_like(xs)
        _check(hip_lib().dm_mace_symc_bwd_f32(
            _fp(go.contiguous()), _fp(xs), _ip(elem), _fp(W), _ip(nz),
            _fp(nzc), nz.numel() // 6, _fp(dx), N, C, T, ctx.S_out,
            _stream()), "dm_mace_symc_bwd_f32")
        return dx, None, None, None, None, None


def symmetric_contract_hip(prod: ProductBasis, x: Dict[int, torch.Tensor],
                           species: torch.Tensor, correlation: int
                           ) -> Dict[int, torch.Tensor]:
    like = next(iter(x.values()))
    N, C = like.shape[0], like.shape[1]
    xs = torch.cat([x[l].permute(0, 2, 1) for l in sorted(x)],
                   dim=1).contiguous()            # [N, 16, C]
    nz, nzc, T, S_out, _ = _symc_nz(tuple(prod.out_ls), correlation,
                                    str(like.device))
    W = _symc_wcat(prod, correlation)
    elem = species.to(torch.int32).contiguous()
    out = _MaceSymcFn.apply(xs, elem, W, nz, nzc, S_out)
    res, off = {}, 0
    for lo in prod.out_ls:
        do = 2 * lo + 1
        res[lo] = out[:, off:off + do, :].permute(0, 2, 1).contiguous()
        off += do
    return res


def symc_hip_available(x: Dict[int, torch.Tensor],
                       prod: ProductBasis) -> bool:
    import os
    like = next(iter(x.values()))
    return (os.environ.get("DM_MACE_SYMC", "hip") == "hip"
            and like.is_cuda and like.shape[1] in (64, 128)
            and sorted(x) == [0, 1, 2, 3]
            and not any(p.requires_grad for p in prod.weights.values()))


# ---------------------------------------------------------------------------
# tree-factored HIP symmetric contraction (csrc/mace_symc.hip): one wave per
# (node, 64-channel block), the polynomial evaluated through its coupling
# trees as two-factor products, any C % 64 == 0.  Same W table, layouts and
# frozen-weight convention as the flat kernel above.
# ---------------------------------------------------------------------------

@lru_cache(maxsize=None)
def _symc_tree_tables(out_ls, correlation: int, device_str: str):
    """The int32 table of dm_mace_symc_tree_* (layout: csrc/mace_symc.hip)
    for the trees of _symc_nz, in its wrow order.  Returns
    (tab, T, S_out, sizes); sizes counts groups, trees, pairs, segs and
    stage-1 / stage-2 / transposed entries."""
    import numpy as np
    assert correlation <= 3, correlation
    ONE = 16                        # the x row that holds 1
    nz, segs, pairs, pair_id = [], [], [], {}

    def add_segs(ents, dsts):
        """ents (dst, p, q, coef) as one seg per dst; -> [beg, end)"""
        beg = len(segs)
        for d in dsts:
            b = len(nz)
            nz.extend(e[1:] for e in ents if e[0] == d)
            segs.append((d, b, len(nz), 0))
        return beg, len(segs)

    def cg_ents(o1, o2, CG):
        return [(o1 + a, o2 + b, m, CG[a, b, m])
                for a, b, m in np.argwhere(np.abs(CG) > 1e-12)]

    def pair(key, ents):
        """stage-1 entries (a, b, mL, coef) of one pair, stored once"""
        if key not in pair_id:
            rp = []
            for m in range(9):
                rp.append(len(nz))
                nz.extend((a, b, c) for a, b, mm, c in ents if mm == m)
            rp.append(len(nz))
            tr = ([(a, m, b, c) for a, b, m, c in ents if a != ONE]
                  + [(b, m, a, c) for a, b, m, c in ents if b != ONE])
            rp.extend(add_segs(tr, sorted({e[0] for e in tr})))
            pair_id[key] = len(pairs)
            pairs.append(rp)
        return pair_id[key]

    groups = {}                     # (lo, L, l3) -> [(wrow, pair)]
    o_offs, wrow, o_off, n_s1 = {}, 0, 0, 0
    for lo in out_ls:
        o_offs[lo] = o_off
        for nu in range(1, correlation + 1):
            for tr in so3.symmetric_basis_trees(nu, lo)[0]:
                if nu == 1:
                    pid = pair((lo,), [(so3.L_OFF[lo] + m, ONE, m, 1.0)
                                       for m in range(2 * lo + 1)])
                    gkey = (lo, lo, None)
                else:
                    l1, l2, L = tr[0], tr[1], (lo if nu == 2 else tr[2])
                    pid = pair((l1, l2, L),
                               cg_ents(so3.L_OFF[l1], so3.L_OFF[l2],
                                       so3.real_cg(l1, l2, L)))
                    gkey = (lo, L, None if nu == 2 else tr[3])
                assert 2 * gkey[1] + 1 <= 9, gkey
                groups.setdefault(gkey, []).append((wrow, pid))
                n_s1 += pairs[pid][9] - pairs[pid][0]
                wrow += 1
        o_off += 2 * lo + 1
    assert o_off <= 4, out_ls
    trees, grows, n_s2 = [], [], 0
    for (lo, L, l3), tl in groups.items():
        if l3 is None:              # identity against the row of ones
            s2 = [(o_offs[lo] + m, m, ONE, 1.0) for m in range(2 * lo + 1)]
        else:
            s2 = [(o_offs[lo] + o, m, so3.L_OFF[l3] + k, c)
                  for m, k, o, c in cg_ents(0, 0, so3.real_cg(L, l3, lo))]
        n_s2 += len(s2)
        row = [len(trees), len(trees) + len(tl)]
        trees.extend(tl)
        row.extend(add_segs([(o, m, k, c) for o, m, k, c in s2],
                            sorted({e[0] for e in s2})))
        row.extend(add_segs([(m, o, k, c) for o, m, k, c in s2],
                            range(2 * L + 1)))
        bk = [(k, o, m, c) for o, m, k, c in s2 if k != ONE]
        row.extend(add_segs(bk, sorted({e[0] for e in bk})))
        grows.append(row)
    ent = np.asarray([(p, q) for p, q, _ in nz], dtype=np.int64)
    assert ent.min() >= 0 and ent.max() <= ONE and len(nz) < 2 ** 31
    assert all(0 <= s[0] < 16 and 0 <= s[1] <= s[2] <= len(nz) for s in segs)
    nzw = np.empty((len(nz), 2), dtype=np.int32)
    nzw[:, 0] = ent[:, 0] | (ent[:, 1] << 8)
    nzw[:, 1] = np.asarray([c for _, _, c in nz], dtype=np.float32) \
        .view(np.int32)
    parts = [np.asarray(a, dtype=np.int32).reshape(-1)
             for a in (grows, trees, pairs, segs)]
    offs = [16]
    for a in parts:
        offs.append(offs[-1] + a.size)
    pad = offs[-1] % 2              # nz is read as int2: 8-byte aligned
    offs[-1] += pad
    head = np.zeros(16, dtype=np.int32)
    head[0], head[1:6] = len(grows), offs
    tab = np.concatenate([head] + parts + [np.zeros(pad, np.int32),
                                           nzw.reshape(-1)])
    sizes = {"groups": len(grows), "trees": len(trees), "pairs": len(pairs),
             "segs": len(segs), "stage1_per_tree": int(n_s1),
             "stage2": n_s2, "nz": len(nz), "int32": int(tab.size)}
    return (torch.tensor(tab, device=torch.device(device_str)), wrow, o_off,
            sizes)


class _MaceSymcTreeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xs, elem, W, tab, S_out):
        from distmlip_amd.ops import _check, _fp, _ip, _stream, hip_lib
        N, _, C = xs.shape
        out = torch.empty(N, S_out, C, dtype=xs.dtype, device=xs.device)
        _check(hip_lib().dm_mace_symc_tree_fwd_f32(
            _fp(xs), _ip(elem), _fp(W), _ip(tab), _fp(out), N, C,
            W.shape[1], S_out, _stream()), "dm_mace_symc_tree_fwd_f32")
        ctx.save_for_backward(xs, elem, W, tab)
        ctx.S_out = S_out
        return out

    @staticmethod
    def backward(ctx, go):
        from distmlip_amd.ops import _check, _fp, _ip, _stream, hip_lib
        xs, elem, W, tab = ctx.saved_tensors
        N, _, C = xs.shape
        dx = torch.empty_like(xs)
        _check(hip_lib().dm_mace_symc_tree_bwd_f32(
            _fp(go.contiguous()), _fp(xs), _ip(elem), _fp(W), _ip(tab),
            _fp(dx), N, C, W.shape[1], ctx.S_out, _stream()),
            "dm_mace_symc_tree_bwd_f32")
        return dx, None, None, None, None


def symmetric_contract_tree(prod: ProductBasis, x: Dict[int, torch.Tensor],
                            species: torch.Tensor, correlation: int
                            ) -> Dict[int, torch.Tensor]:
    like = next(iter(x.values()))
    xs = torch.cat([x[l].permute(0, 2, 1) for l in sorted(x)],
                   dim=1).contiguous()            # [N, 16, C]
    tab, T, S_out, _ = _symc_tree_tables(tuple(prod.out_ls), correlation,
                                         str(like.device))
    W = _symc_wcat(prod, correlation)
    assert W.shape[1] == T and xs.shape[1] == 16, (W.shape, xs.shape)
    elem = species.to(torch.int32).contiguous()
    out = _MaceSymcTreeFn.apply(xs, elem, W, tab, S_out)
    res, off = {}, 0
    for lo in prod.out_ls:
        do = 2 * lo + 1
        res[lo] = out[:, off:off + do, :].permute(0, 2, 1).contiguous()
        off += do
    return res


def symc_tree_available(x: Dict[int, torch.Tensor],
                        prod: ProductBasis) -> bool:
    """DM_MACE_SYMC=tree, or unset / hip at a width the flat kernel does
    not serve; torch pins the composition."""
    import os
    like = next(iter(x.values()))
    return (os.environ.get("DM_MACE_SYMC", "hip") in ("hip", "tree")
            and like.is_cuda and like.dtype == torch.float32
            and like.shape[1] > 0 and like.shape[1] % 64 == 0
            and sorted(x) == [0, 1, 2, 3]
            and sum(2 * lo + 1 for lo in prod.out_ls) <= 4
            and not any(p.requires_grad for p in prod.weights.values()))
