"""TensorNet arithmetic — the forwards both drivers share
(tensornet.TensorNet_Dist and tensornet_runtime.TensorNetSpmdEngine), over
the ops backend (distmlip_amd.ops_base).

Layout: node tensors are component-major, T[n, 3a+b, c] ("T9"); per-edge
radial weights are f[e, k, c], k in (I, A, S).  Node-level algebra stays in
torch: channel mixes are one tall [N*9, C] x [C, C] GEMM, and the 3x3
products are written as multiply-adds over [N, C] planes — never bmm/matmul
on 3x3 tiles, which rocBLAS runs as millions of tiny batched GEMMs
(mace_ops.conv_tp_messages records the measurement).

The one irregular op is the message pass
    M[i,:,c] = sum_{e -> i} sum_k f[e,k,c] * P_k(Y[src[e],:,c])
`tn_message` is its torch composition over ops.gather / ops.scatter_edges
(CPU and fallback path; it materialises [E, 9, C] three times);
`tn_message_hip` is one autograd.Function over the three fused gfx950
kernels of include/distmlip_hip.h (dm_tn_msg_*), which never do.
DM_TN_MSG=torch forces the composition for A/B runs.
"""
from __future__ import annotations

import math
import os

import torch
import torch.nn.functional as F

from distmlip_amd.tensornet_model import Interaction, TensorNetCore

_DIAG = (0, 4, 8)


# -- 3x3 algebra on [*, 9, C] planes -----------------------------------------

def tnorm(T9: torch.Tensor) -> torch.Tensor:
    """Sum over the nine entries of T^2 (no square root) -> [*, C]."""
    return (T9 * T9).sum(dim=1)


def dec9(T9: torch.Tensor):
    """(I, A, S) parts of T, each [*, 9, C]:
    I = tr(T)/3 * 1, A = (T - T^T)/2, S = (T + T^T)/2 - I."""
    t = T9.unbind(dim=1)
    tr3 = (t[0] + t[4] + t[8]) / 3.0
    z = torch.zeros_like(tr3)
    a01, a02, a12 = 0.5 * (t[1] - t[3]), 0.5 * (t[2] - t[6]), \
        0.5 * (t[5] - t[7])
    s01, s02, s12 = 0.5 * (t[1] + t[3]), 0.5 * (t[2] + t[6]), \
        0.5 * (t[5] + t[7])
    I = torch.stack((tr3, z, z, z, tr3, z, z, z, tr3), dim=1)
    A = torch.stack((z, a01, a02, -a01, z, a12, -a02, -a12, z), dim=1)
    S = torch.stack((t[0] - tr3, s01, s02, s01, t[4] - tr3, s12,
                     s02, s12, t[8] - tr3), dim=1)
    return I, A, S


def _sum3(a, b, c):
    """a + b + c with both additions' rounding errors added back (TwoSum):
    accurate relative to |a + b + c| even when the terms cancel."""
    s1 = a + b
    b1 = s1 - a
    e1 = (a - (s1 - b1)) + (b - b1)
    s2 = s1 + c
    b2 = s2 - s1
    e2 = (s1 - (s2 - b2)) + (c - b2)
    return s2 + (e1 + e2)


def dec9_acc(T9: torch.Tensor):
    """dec9 with every part accurate relative to itself (the trace and the
    diagonal of S through _sum3), as the fused kernels form them.  Not for
    autograd: used inside _ProjectFn, which writes its own reverse."""
    t = T9.unbind(dim=1)
    tr3 = _sum3(t[0], t[4], t[8]) / 3.0
    sd = (_sum3(2.0 * t[0], -t[4], -t[8]) / 3.0,
          _sum3(2.0 * t[4], -t[0], -t[8]) / 3.0,
          _sum3(2.0 * t[8], -t[0], -t[4]) / 3.0)
    z = torch.zeros_like(tr3)
    a01, a02, a12 = 0.5 * (t[1] - t[3]), 0.5 * (t[2] - t[6]), \
        0.5 * (t[5] - t[7])
    s01, s02, s12 = 0.5 * (t[1] + t[3]), 0.5 * (t[2] + t[6]), \
        0.5 * (t[5] + t[7])
    I = torch.stack((tr3, z, z, z, tr3, z, z, z, tr3), dim=1)
    A = torch.stack((z, a01, a02, -a01, z, a12, -a02, -a12, z), dim=1)
    S = torch.stack((sd[0], s01, s02, s01, sd[1], s12, s02, s12, sd[2]),
                    dim=1)
    return I, A, S


def matmul9(A9: torch.Tensor, B9: torch.Tensor) -> torch.Tensor:
    """Per node and channel 3x3 product, plane-wise:
    out[3a+b] = sum_k A[3a+k] * B[3k+b]."""
    a, b = A9.unbind(dim=1), B9.unbind(dim=1)
    return torch.stack(
        [a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j]
         for i in range(3) for j in range(3)], dim=1)


def mix(lin, T9: torch.Tensor) -> torch.Tensor:
    """Bias-free channel mix sum_c W[m,c] T[n,:,c] as one tall GEMM."""
    n, _, C = T9.shape
    return (T9.reshape(n * 9, C) @ lin.weight.t()).view(n, 9, C)


def mix3(lins, I, A, S) -> torch.Tensor:
    return mix(lins[0], I) + mix(lins[1], A) + mix(lins[2], S)


# -- edge basis ----------------------------------------------------------------

def edge_basis(vec: torch.Tensor, core: TensorNetCore):
    """(vhat [E,3], rbf [E,R], cut [E]) of the edge vectors."""
    cfg = core.config
    d = torch.linalg.norm(vec, dim=1)
    vhat = vec / d.unsqueeze(1)
    mu = torch.linspace(0.0, cfg.cutoff, cfg.num_rbf, dtype=d.dtype,
                        device=d.device)
    rbf = torch.exp(-cfg.rbf_width * (d.unsqueeze(1) - mu) ** 2)
    cut = 0.5 * (torch.cos(d * (math.pi / cfg.cutoff)) + 1.0)
    cut = torch.where(d < cfg.cutoff, cut, torch.zeros_like(cut))
    return vhat, rbf, cut


def _edge_tensors(vhat: torch.Tensor):
    """skew(v) and v v^T - 1/3 as [E, 9] rows (row order 3a+b)."""
    x, y, z = vhat.unbind(dim=1)
    o = torch.zeros_like(x)
    skew = torch.stack((o, -z, y, z, o, -x, -y, x, o), dim=1)
    third = 1.0 / 3.0
    sym = torch.stack((x * x - third, x * y, x * z,
                       y * x, y * y - third, y * z,
                       z * x, z * y, z * z - third), dim=1)
    return skew, sym


# -- message pass ----------------------------------------------------------------

def _src_csr(pd):
    return (pd.src_perm, pd.src_row_ptr) if hasattr(pd, "src_perm") else None


class _ProjectFn(torch.autograd.Function):
    """msg[e,:,c] = sum_k f[e,k,c] * P_k(g[e,:,c]) on [E,9,C] rows, with the
    reverse the fused kernels use (the projections are self-adjoint):
    dg = sum_k f_k P_k(gm), df_k = <gm, P_k(g)>."""

    @staticmethod
    def forward(ctx, g, f):
        ctx.save_for_backward(g, f)
        I, A, S = dec9_acc(g)
        return I * f[:, 0:1] + A * f[:, 1:2] + S * f[:, 2:3]

    @staticmethod
    def backward(ctx, gm):
        g, f = ctx.saved_tensors
        I, A, S = dec9_acc(gm)
        dg = I * f[:, 0:1] + A * f[:, 1:2] + S * f[:, 2:3]
        df = torch.stack([(gm * p).sum(dim=1) for p in dec9_acc(g)], dim=1)
        return dg, df


def tn_message(Y: torch.Tensor, f: torch.Tensor, pd, ops) -> torch.Tensor:
    """Torch composition of the message pass: gather Y[src] to [E,9,C],
    project, scale by f [E,3,C], segment-sum at dst -> [N,9,C]."""
    n, _, C = Y.shape
    g = ops.gather(Y.reshape(n, 9 * C), pd.src, csr=_src_csr(pd))
    msg = _ProjectFn.apply(g.view(-1, 9, C), f)
    return ops.scatter_edges(msg.reshape(-1, 9 * C).contiguous(),
                             pd).view(n, 9, C)


class _TnMessageFn(torch.autograd.Function):
    """M = message pass of (Y [N,9,C], f [E,3,C]); forward one kernel over
    the dst CSR, backward one kernel per gradient (df over the dst CSR, dY
    over the src permutation CSR).  Deterministic: no atomics."""

    @staticmethod
    def forward(ctx, Y, f, src, dst, row_ptr, src_perm, src_row_ptr):
        from distmlip_amd.ops import _check, _chk_f32, _fp, _ip, _stream, \
            hip_lib
        _chk_f32(Y, f)
        N, _, C = Y.shape
        ctx.save_for_backward(Y, f)
        ctx.idx = (src, dst, row_ptr, src_perm, src_row_ptr)
        if f.shape[0] == 0:
            return torch.zeros_like(Y)
        M = torch.empty_like(Y)
        _check(hip_lib().dm_tn_msg_fwd_f32(
            _fp(Y), _fp(f), _ip(src), _ip(row_ptr), _fp(M), N, C,
            _stream()), "dm_tn_msg_fwd_f32")
        return M

    @staticmethod
    def backward(ctx, G):
        from distmlip_amd.ops import _check, _fp, _ip, _stream, hip_lib
        Y, f = ctx.saved_tensors
        src, dst, row_ptr, src_perm, src_row_ptr = ctx.idx
        N, _, C = Y.shape
        dY = df = None
        if f.shape[0] == 0:
            return (torch.zeros_like(Y), torch.zeros_like(f),
                    None, None, None, None, None)
        G = G.contiguous()
        if ctx.needs_input_grad[0]:
            dY = torch.empty_like(Y)
            _check(hip_lib().dm_tn_msg_bwd_node_f32(
                _fp(G), _fp(f), _ip(dst), _ip(src_perm), _ip(src_row_ptr),
                _fp(dY), N, C, _stream()), "dm_tn_msg_bwd_node_f32")
        if ctx.needs_input_grad[1]:
            df = torch.empty_like(f)
            _check(hip_lib().dm_tn_msg_bwd_edge_f32(
                _fp(G), _fp(Y), _ip(src), _ip(row_ptr), _fp(df), N, C,
                _stream()), "dm_tn_msg_bwd_edge_f32")
        return dY, df, None, None, None, None, None


def tn_message_hip_available(Y: torch.Tensor, f: torch.Tensor, pd,
                             ops) -> bool:
    return (os.environ.get("DM_TN_MSG", "hip") == "hip"
            and Y.is_cuda and f.is_cuda
            and Y.dtype == torch.float32 and f.dtype == torch.float32
            and Y.shape[-1] % 64 == 0
            and not getattr(ops, "is_reference", False)
            and hasattr(pd, "src_perm"))


def tn_message_hip(Y: torch.Tensor, f: torch.Tensor, pd) -> torch.Tensor:
    """Fused message pass (see _TnMessageFn); pd carries the int32 dst CSR
    and src permutation CSR of the graph builder."""
    return _TnMessageFn.apply(Y.contiguous(), f.contiguous(), pd.src, pd.dst,
                              pd.row_ptr, pd.src_perm, pd.src_row_ptr)


def message(Y, f, pd, ops):
    if tn_message_hip_available(Y, f, pd, ops):
        return tn_message_hip(Y, f, pd)
    return tn_message(Y, f, pd, ops)


# -- model forwards ----------------------------------------------------------------

def tn_embedding(core: TensorNetCore, species: torch.Tensor, vhat, rbf, cut,
                 pd, ops) -> torch.Tensor:
    """matgl TensorEmbedding: X [n, 9, C] from species and edge geometry.
    Runs once per step, so the accumulate is [E, 9C] coefficient rows through
    the backend's segment sum, not a fused kernel."""
    emb = core.embedding
    C = core.config.units
    n = species.shape[0]
    src, dst = pd.src.long(), pd.dst.long()
    with torch.no_grad():                   # species only: no gradient
        x = emb.emb(species)
        Z = emb.pair(torch.cat((x[src], x[dst]), dim=1))
    cz = cut.unsqueeze(1) * Z
    wI, wA, wS = emb.rbf_I(rbf) * cz, emb.rbf_A(rbf) * cz, emb.rbf_S(rbf) * cz
    skew, sym = _edge_tensors(vhat)
    eye = skew.new_zeros(9)
    eye[list(_DIAG)] = 1.0
    coef = (eye.view(1, 9, 1) * wI.unsqueeze(1)
            + skew.unsqueeze(2) * wA.unsqueeze(1)
            + sym.unsqueeze(2) * wS.unsqueeze(1))
    X0 = ops.scatter_edges(coef.reshape(-1, 9 * C).contiguous(),
                           pd).view(n, 9, C)
    I, A, S = dec9(X0)          # the three sums: the parts of their total
    nrm = F.layer_norm(tnorm(X0), (C,), emb.norm.weight, emb.norm.bias,
                       emb.norm.eps)
    I, A, S = mix(emb.mix[0], I), mix(emb.mix[1], A), mix(emb.mix[2], S)
    nrm = F.silu(emb.scalar1(nrm))
    nrm = F.silu(emb.scalar2(nrm)).view(n, 3, C)
    return I * nrm[:, 0:1] + A * nrm[:, 1:2] + S * nrm[:, 2:3]


def tn_edge_weights(layer: Interaction, rbf, cut) -> torch.Tensor:
    """f [E, 3, C]: the layer's radial MLP times the cutoff."""
    f = F.silu(layer.edge1(rbf))
    f = F.silu(layer.edge2(f))
    f = F.silu(layer.edge3(f)) * cut.unsqueeze(1)
    return f.view(f.shape[0], 3, -1)


def tn_layer(layer: Interaction, X: torch.Tensor, rbf, cut, pd, ops,
             group: str = "O(3)") -> torch.Tensor:
    """matgl TensorNetInteraction on the local nodes of one partition."""
    f = tn_edge_weights(layer, rbf, cut)
    X = X / (tnorm(X) + 1.0).unsqueeze(1)
    Y = mix3(layer.mix[0:3], *dec9(X))
    M = message(Y, f, pd, ops)
    if group == "O(3)":
        T = matmul9(M, Y) + matmul9(Y, M)
    else:
        T = 2.0 * matmul9(Y, M)
    I, A, S = dec9(T)
    inv = (1.0 / (tnorm(T) + 1.0)).unsqueeze(1)
    dX = mix3(layer.mix[3:6], I * inv, A * inv, S * inv)
    return X + dX + matmul9(dX, dX)


def tn_node_energy(core: TensorNetCore, X: torch.Tensor) -> torch.Tensor:
    """Extensive readout: per-node energies [n] (summed by the caller over
    the atoms it owns)."""
    if core.config.is_intensive:
        raise NotImplementedError(
            "is_intensive = True is not supported by distributed inference")
    C = core.config.units
    I, A, S = dec9(X)
    x = torch.cat((tnorm(I), tnorm(A), tnorm(S)), dim=-1)
    x = F.layer_norm(x, (3 * C,), core.out_norm.weight, core.out_norm.bias,
                     core.out_norm.eps)
    return core.final_layer(core.linear(x)).squeeze(-1)
