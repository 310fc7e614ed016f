"""Independent TensorNet oracle (test helper, not a test module).

A dense restatement on [N, C, 3, 3] tensors with index_add, written
straight from the model definition; fp64-capable.  It shares no code with
distmlip_amd.tensornet_ops / tensornet_model beyond reading the core's
weights, and it undoes the k-major row order of the two ->3C linears
itself, back to matgl's channel-major reshape(-1, C, 3).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def _tnorm(T):
    return (T ** 2).sum((-2, -1))


def _dec(T):
    eye = torch.eye(3, dtype=T.dtype, device=T.device)
    I = T.diagonal(dim1=-2, dim2=-1).mean(-1)[..., None, None] * eye
    A = 0.5 * (T - T.transpose(-2, -1))
    S = 0.5 * (T + T.transpose(-2, -1)) - I
    return I, A, S


def _mix(lin, T):
    # sum_c W[m,c] T[n,c,:,:]
    return torch.einsum("mc,ncab->nmab", lin.weight, T)


def _channel_major(lin, C):
    """(W, b) of a ->3C linear with rows in matgl order c*3 + k."""
    W, b = lin.weight, lin.bias
    Wm = W.view(3, C, -1).permute(1, 0, 2).reshape(3 * C, -1)
    bm = b.view(3, C).t().reshape(3 * C)
    return Wm, bm


def _skew(v):
    o = torch.zeros_like(v[:, 0])
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return torch.stack((torch.stack((o, -z, y), -1),
                        torch.stack((z, o, -x), -1),
                        torch.stack((-y, x, o), -1)), -2)


def message_dense(Y, f, src, dst, n):
    """M_i = sum_{e->i} sum_k f[e,k,:] P_k(Y_src(e)); Y [N,C,3,3],
    f [E,C,3] (channel-major, part last)."""
    I, A, S = _dec(Y[src])
    msg = (f[..., 0, None, None] * I + f[..., 1, None, None] * A
           + f[..., 2, None, None] * S)
    return torch.zeros((n,) + tuple(Y.shape[1:]), dtype=Y.dtype,
                       device=Y.device).index_add_(0, dst, msg)


def tensornet_oracle_forward(core, structure, src, dst, offsets,
                             dtype=torch.float64, compute_forces=True,
                             compute_stress=False):
    cfg = core.config
    C = cfg.units
    lat0 = torch.tensor(np.asarray(structure.lattice), dtype=dtype)
    strain = torch.zeros(3, 3, dtype=dtype)
    if compute_stress:
        strain.requires_grad_(True)
    lattice = lat0 @ (torch.eye(3, dtype=dtype) + strain)
    pos = torch.tensor(np.asarray(structure.frac_coords), dtype=dtype) @ lattice
    if compute_forces and not pos.requires_grad:
        pos.requires_grad_(True)
    z = torch.tensor(np.asarray(structure.species), dtype=torch.long)
    src = torch.as_tensor(np.asarray(src), dtype=torch.long)
    dst = torch.as_tensor(np.asarray(dst), dtype=torch.long)
    off = torch.tensor(np.asarray(offsets), dtype=dtype)
    n = pos.shape[0]

    vec = pos[dst] + off @ lattice - pos[src]
    d = vec.norm(dim=1)
    vhat = vec / d[:, None]
    mu = torch.linspace(0.0, cfg.cutoff, cfg.num_rbf, dtype=dtype)
    rbf = torch.exp(-cfg.rbf_width * (d[:, None] - mu) ** 2)
    cut = torch.where(d < cfg.cutoff,
                      0.5 * (torch.cos(math.pi * d / cfg.cutoff) + 1.0),
                      torch.zeros_like(d))

    # ---- embedding
    emb = core.embedding
    x = emb.emb(z)
    Z = emb.pair(torch.cat((x[src], x[dst]), dim=-1))
    eye = torch.eye(3, dtype=dtype)
    W1 = emb.rbf_I(rbf) * cut[:, None]
    W2 = emb.rbf_A(rbf) * cut[:, None]
    W3 = emb.rbf_S(rbf) * cut[:, None]
    zero = torch.zeros(n, C, 3, 3, dtype=dtype)
    I = zero.index_add(0, dst, (Z * W1)[..., None, None] * eye)
    A = zero.index_add(0, dst, (Z * W2)[..., None, None]
                       * _skew(vhat)[:, None])
    sym = vhat[:, :, None] * vhat[:, None, :] - eye / 3.0
    S = zero.index_add(0, dst, (Z * W3)[..., None, None] * sym[:, None])
    nrm = F.layer_norm(_tnorm(I + A + S), (C,), emb.norm.weight,
                       emb.norm.bias, emb.norm.eps)
    I, A, S = _mix(emb.mix[0], I), _mix(emb.mix[1], A), _mix(emb.mix[2], S)
    nrm = F.silu(emb.scalar1(nrm))
    Wm, bm = _channel_major(emb.scalar2, C)
    nrm = F.silu(F.linear(nrm, Wm, bm)).reshape(-1, C, 3)
    X = (I * nrm[..., 0, None, None] + A * nrm[..., 1, None, None]
         + S * nrm[..., 2, None, None])

    # ---- interaction layers
    for layer in core.layers:
        f = F.silu(layer.edge1(rbf))
        f = F.silu(layer.edge2(f))
        Wm, bm = _channel_major(layer.edge3, C)
        f = F.silu(F.linear(f, Wm, bm))
        f = (f * cut[:, None]).reshape(-1, C, 3)
        X = X / (_tnorm(X) + 1.0)[..., None, None]
        I, A, S = _dec(X)
        Y = _mix(layer.mix[0], I) + _mix(layer.mix[1], A) \
            + _mix(layer.mix[2], S)
        M = message_dense(Y, f, src, dst, n)
        if cfg.group == "O(3)":
            T = torch.matmul(M, Y) + torch.matmul(Y, M)
        else:
            T = 2.0 * torch.matmul(Y, M)
        I, A, S = _dec(T)
        den = (_tnorm(I + A + S) + 1.0)[..., None, None]
        dX = _mix(layer.mix[3], I / den) + _mix(layer.mix[4], A / den) \
            + _mix(layer.mix[5], S / den)
        X = X + dX + torch.matmul(dX, dX)

    # ---- readout
    I, A, S = _dec(X)
    h = torch.cat((_tnorm(I), _tnorm(A), _tnorm(S)), dim=-1)
    h = F.layer_norm(h, (3 * C,), core.out_norm.weight, core.out_norm.bias,
                     core.out_norm.eps)
    e_atoms = core.final_layer(core.linear(h)).squeeze(-1)
    energy = core.data_std * e_atoms.sum() + core.data_mean \
        + core.element_refs[z].sum()

    out = {"energy": energy.detach(), "forces": None, "stress": None}
    if compute_forces:
        grads = [pos, strain] if compute_stress else [pos]
        gv = torch.autograd.grad(energy, grads)
        out["forces"] = -gv[0]
        if compute_stress:
            volume = abs(np.linalg.det(np.asarray(structure.lattice)))
            out["stress"] = -gv[1] / volume * -160.21766208
    return out
