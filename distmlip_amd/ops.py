"""HipOps — the product ops backend over the gfx950 C-ABI kernel library.

Every primitive is a torch.autograd.Function whose forward AND backward are
hand-written HIP kernels (include/distmlip_hip.h); backward scatters run
over the builder's permutation CSRs, so gradients are deterministic (no
atomics).  The dense GEMMs of the gated MLPs stay in rocBLAS via
torch.matmul — this module covers the irregular ops the reference
delegates to DGL.

Fails loudly if the extension is missing or tensors are not fp32 on a HIP
device — there is no fallback.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int32, c_int64, c_uint64

import torch

from distmlip_amd.capi import _load

_hip_lib = None


def hip_lib() -> ctypes.CDLL:
    global _hip_lib
    if _hip_lib is None:
        lib = _load("libdistmlip_hip.so")
        fp = POINTER(c_float)
        ip = POINTER(c_int32)
        lib.dm_gather_rows_f32.restype = c_int32
        lib.dm_gather_rows_f32.argtypes = [fp, ip, fp, c_int64, c_int64, c_uint64]
        lib.dm_gather_add3_f32.restype = c_int32
        lib.dm_gather_add3_f32.argtypes = [fp, fp, fp, ip, ip, fp, fp,
                                           c_int64, c_int64, c_uint64]
        lib.dm_gather_add4_f32.restype = c_int32
        lib.dm_gather_add4_f32.argtypes = [fp, fp, fp, fp, ip, ip, ip, fp,
                                           fp, c_int64, c_int64, c_uint64]
        lib.dm_edge_mlp3_f32.restype = c_int32
        lib.dm_edge_mlp3_f32.argtypes = [fp, fp, fp, fp, fp, ip, ip, fp, fp,
                                         c_int64, c_int64, c_int64, c_uint64]
        lib.dm_edge_mlp4_f32.restype = c_int32
        lib.dm_edge_mlp4_f32.argtypes = [fp, fp, fp, fp, fp, fp, ip, ip, ip,
                                         fp, fp, c_int64, c_int64, c_int64,
                                         c_uint64]
        lib.dm_silu_bwd_f32.restype = c_int32
        lib.dm_silu_bwd_f32.argtypes = [fp, fp, fp, fp, c_int64, c_uint64]
        lib.dm_seg_sum_f32.restype = c_int32
        lib.dm_seg_sum_f32.argtypes = [fp, ip, fp, fp, c_int64, c_int64,
                                       c_uint64]
        lib.dm_seg_sum_gather_f32.restype = c_int32
        lib.dm_seg_sum_gather_f32.argtypes = [fp, ip, ip, fp, fp, c_int64,
                                              c_int64, c_uint64]
        lib.dm_gated_combine_fwd_f32.restype = c_int32
        lib.dm_gated_combine_fwd_f32.argtypes = [fp, fp, fp, fp, fp, c_int64,
                                                 c_uint64]
        lib.dm_gated_combine_bwd_f32.restype = c_int32
        lib.dm_gated_combine_bwd_f32.argtypes = [fp, fp, fp, fp, fp, fp, fp,
                                                 c_int64, c_uint64]
        lib.dm_gated_mlp_tail_bwd_f32.restype = c_int32
        lib.dm_gated_mlp_tail_bwd_f32.argtypes = [fp, fp, fp, fp, fp, fp, fp,
                                                  fp, fp, c_int64, c_int64,
                                                  c_uint64]
        lib.dm_gated_mlp_tail_bwd_idx_f32.restype = c_int32
        lib.dm_gated_mlp_tail_bwd_idx_f32.argtypes = [fp, ip, fp, fp, fp, fp,
                                                      fp, fp, fp, fp, c_int64,
                                                      c_int64, c_uint64]
        lib.dm_edge_mlp_bwd_f32.restype = c_int32
        lib.dm_edge_mlp_bwd_f32.argtypes = [fp, fp, fp, fp, c_int64, c_int64,
                                            c_int64, c_uint64]
        lib.dm_gated_mlp_tail_fwd_f32.restype = c_int32
        lib.dm_gated_mlp_tail_fwd_f32.argtypes = [fp, fp, fp, fp, fp, fp, fp,
                                                  fp, fp, fp, c_int64,
                                                  c_int64, c_uint64]
        lib.dm_gated_mlp3_f32.restype = c_int32
        lib.dm_gated_mlp3_f32.argtypes = [fp, fp, fp, fp, fp, ip, ip, fp, fp,
                                          fp, fp, fp, fp, fp, fp, fp, fp,
                                          c_int64, c_int64, c_int64, c_uint64]
        lib.dm_gated_mlp4_f32.restype = c_int32
        lib.dm_gated_mlp4_f32.argtypes = [fp, fp, fp, fp, fp, fp, ip, ip, ip,
                                          fp, fp, fp, fp, fp, fp, fp, fp, fp,
                                          fp, c_int64, c_int64, c_int64,
                                          c_uint64]
        # factored message weight (RadialW): bexp, W, mask in place of w
        lib.dm_gated_mlp_tail_fwd_fw_f32.restype = c_int32
        lib.dm_gated_mlp_tail_fwd_fw_f32.argtypes = [
            fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, c_int64, c_int64,
            c_int64, c_uint64]
        lib.dm_gated_mlp3_fw_f32.restype = c_int32
        lib.dm_gated_mlp3_fw_f32.argtypes = [
            fp, fp, fp, fp, fp, ip, ip, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp,
            fp, fp, c_int64, c_int64, c_int64, c_int64, c_uint64]
        lib.dm_gated_mlp_tail_bwd_fw_f32.restype = c_int32
        lib.dm_gated_mlp_tail_bwd_fw_f32.argtypes = [
            fp, ip, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, c_int64,
            c_int64, c_int64, c_uint64]
        lib.dm_mace_tp_fwd_f32.restype = c_int32
        lib.dm_mace_tp_fwd_f32.argtypes = [fp, fp, fp, fp, ip, fp, c_int32,
                                           fp, fp, fp, fp, c_int64, c_int32,
                                           c_int32, c_int32, c_uint64]
        lib.dm_rot_gather_f32.restype = c_int32
        lib.dm_rot_gather_f32.argtypes = [fp, ip, fp, c_int32, fp,
                                          c_int64, c_int32, c_uint64]
        lib.dm_rot_scatter_f32.restype = c_int32
        lib.dm_rot_scatter_f32.argtypes = [fp, fp, c_int32, ip, ip, fp,
                                           fp, c_int64, c_int32, c_uint64]
        lib.dm_rot_dD_f32.restype = c_int32
        lib.dm_rot_dD_f32.argtypes = [fp, fp, ip, c_int32, fp, c_int64,
                                      c_int32, c_uint64]
        lib.dm_mace_symc_fwd_f32.restype = c_int32
        lib.dm_mace_symc_fwd_f32.argtypes = [fp, ip, fp, ip, fp, c_int32,
                                             fp, c_int64, c_int32, c_int32,
                                             c_int32, c_uint64]
        lib.dm_mace_symc_bwd_f32.restype = c_int32
        lib.dm_mace_symc_bwd_f32.argtypes = [fp, fp, ip, fp, ip, fp,
                                             c_int32, fp, c_int64, c_int32,
                                             c_int32, c_int32, c_uint64]
        lib.dm_mace_tp_bwd_f32.restype = c_int32
        lib.dm_mace_tp_bwd_f32.argtypes = [fp, fp, fp, fp, fp, fp, fp, fp,
                                           ip, fp, c_int32, fp, fp, fp, fp,
                                           c_int64, c_int32, c_int32,
                                           c_int32, c_uint64]
        # TensorNet message pass (distmlip_amd/tensornet_ops.py)
        lib.dm_tn_msg_fwd_f32.restype = c_int32
        lib.dm_tn_msg_fwd_f32.argtypes = [fp, fp, ip, ip, fp, c_int64,
                                          c_int32, c_uint64]
        lib.dm_tn_msg_bwd_edge_f32.restype = c_int32
        lib.dm_tn_msg_bwd_edge_f32.argtypes = [fp, fp, ip, ip, fp, c_int64,
                                               c_int32, c_uint64]
        lib.dm_tn_msg_bwd_node_f32.restype = c_int32
        lib.dm_tn_msg_bwd_node_f32.argtypes = [fp, fp, ip, ip, ip, fp,
                                               c_int64, c_int32, c_uint64]
        cf = ctypes.c_float
        lib.dm_edge_geom_rbf_fwd_f32.restype = c_int32
        lib.dm_edge_geom_rbf_fwd_f32.argtypes = [fp, ip, ip, fp, fp, cf,
                                                 c_int32, c_int32, fp, fp, fp,
                                                 c_int64, c_uint64]
        lib.dm_edge_geom_rbf_bwd_f32.restype = c_int32
        lib.dm_edge_geom_rbf_bwd_f32.argtypes = [fp, fp, fp, fp, fp, fp, cf,
                                                 c_int32, c_int32, fp,
                                                 c_int64, c_uint64]
        lib.dm_rbf_env_fwd_f32.restype = c_int32
        lib.dm_rbf_env_fwd_f32.argtypes = [fp, fp, cf, c_int32, c_int32, fp,
                                           c_int64, c_uint64]
        lib.dm_rbf_env_bwd_f32.restype = c_int32
        lib.dm_rbf_env_bwd_f32.argtypes = [fp, fp, fp, cf, c_int32, c_int32,
                                           fp, c_int64, c_uint64]
        dp = POINTER(ctypes.c_double)
        cd = ctypes.c_double
        # pos, cid, order, cell_start | host: lattice9, nc3, R3, pbc3
        nl_gen = [dp, ip, ip, ip, dp, ip, ip, ip]
        lib.dm_nl_count_gen_f64.restype = c_int32
        lib.dm_nl_count_gen_f64.argtypes = nl_gen + [cd, cd, ip, c_int64,
                                                     c_uint64]
        lib.dm_nl_fill_gen_f64.restype = c_int32
        lib.dm_nl_fill_gen_f64.argtypes = nl_gen + [
            cd, cd, cd, ip, ip, POINTER(ctypes.c_int8),
            POINTER(ctypes.c_uint8), c_int64, c_uint64]
        # MD integrator kernels (distmlip_amd/md_ops.py)
        vp = ctypes.c_void_p
        # frac, vel, force, force_f64, inv_mass, xi | a, b, h, c1, c2 |
        # host: linv9, pbc3
        lib.dm_md_kick_drift_f64.restype = c_int32
        lib.dm_md_kick_drift_f64.argtypes = [dp, dp, vp, c_int32, dp, dp,
                                             cd, cd, cd, cd, cd, dp, ip,
                                             c_int64, c_uint64]
        lib.dm_md_kick_reduce_f64.restype = c_int32
        lib.dm_md_kick_reduce_f64.argtypes = [dp, vp, c_int32, dp, cd, dp,
                                              dp, c_int64, c_uint64]
        # indexed row moves (csrc/rows.hip): src, si, dst, di, M, D, op
        lp = POINTER(c_int64)
        lib.dm_move_rows_f32.restype = c_int32
        lib.dm_move_rows_f32.argtypes = [fp, lp, fp, lp, c_int64, c_int64,
                                         c_int32, c_uint64]
        lib.dm_zero_rows_f32.restype = c_int32
        lib.dm_zero_rows_f32.argtypes = [fp, lp, c_int64, c_int64, c_uint64]
        # exact sigmoid / SiLU: check against the plain expressions, evaluate
        up = POINTER(ctypes.c_uint32)
        lib.dm_act_check_f32.restype = c_int32
        lib.dm_act_check_f32.argtypes = [c_int32, ctypes.c_uint32, c_uint64,
                                         up, up, c_uint64]
        lib.dm_act_eval_f32.restype = c_int32
        lib.dm_act_eval_f32.argtypes = [c_int32, c_int32, fp, c_int64, fp,
                                        c_uint64]
        lib.dm_hip_last_error.restype = c_char_p
        _hip_lib = lib
    return _hip_lib


def _fp(t):
    return ctypes.cast(t.data_ptr(), POINTER(c_float))


def _ip(t):
    return ctypes.cast(t.data_ptr(), POINTER(c_int32))


def _stream():
    return c_uint64(torch.cuda.current_stream().cuda_stream)


def _check(rc: int, name: str):
    if rc != 0:
        raise RuntimeError(f"{name} failed: {hip_lib().dm_hip_last_error().decode()}")


def _chk_f32(*ts):
    for t in ts:
        if t is None:
            continue
        if t.device.type != "cuda":
            raise RuntimeError("HipOps requires device tensors (got CPU); "
                               "the product path has no CPU fallback")
        assert t.dtype == torch.float32 and t.is_contiguous()


def raw_gather(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    _chk_f32(x)
    out = torch.empty((idx.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype,
                      device=x.device)
    _check(hip_lib().dm_gather_rows_f32(
        _fp(x), _ip(idx), _fp(out), out.shape[0], x.shape[1], _stream()),
        "dm_gather_rows_f32")
    return out


def _lp(t):
    return ctypes.cast(t.data_ptr(), POINTER(c_int64)) if t is not None \
        else None


def _chk_rows(t, idx, M):
    """t is a [R, D] fp32 device array; idx an int64 [M] device index into its
    rows, or None for rows 0..M-1."""
    _chk_f32(t)
    assert t.dim() == 2
    if idx is None:
        assert M <= t.shape[0]
    else:
        assert idx.dtype == torch.int64 and idx.is_contiguous() \
            and idx.device == t.device and idx.shape == (M,)


def raw_move_rows(src, si, dst, di, add=False):
    """dst[di[i]] (=|+=) src[si[i]] for every i, IN PLACE over dst, one
    kernel.  si / di: int64 [M] or None for the identity; the entries of di
    must be unique and every index a valid row (not checked: that would cost
    a device round trip).  src and dst must not overlap."""
    M = len(si) if si is not None else len(di) if di is not None \
        else src.shape[0]
    _chk_rows(src, si, M)
    _chk_rows(dst, di, M)
    assert src.shape[1] == dst.shape[1]
    _check(hip_lib().dm_move_rows_f32(
        _fp(src), _lp(si), _fp(dst), _lp(di), M, src.shape[1],
        1 if add else 0, _stream()), "dm_move_rows_f32")
    return dst


def raw_zero_rows(dst, di, M=None):
    """dst[di[i]] = 0 for every i, IN PLACE, one kernel; di None: the first
    M rows."""
    M = len(di) if di is not None else M
    _chk_rows(dst, di, M)
    _check(hip_lib().dm_zero_rows_f32(
        _fp(dst), _lp(di), M, dst.shape[1], _stream()), "dm_zero_rows_f32")
    return dst


def raw_seg_sum(msg, row_ptr, n_rows, base=None):
    _chk_f32(msg, base)
    out = torch.empty((n_rows,) + tuple(msg.shape[1:]), dtype=msg.dtype,
                      device=msg.device)
    _check(hip_lib().dm_seg_sum_f32(
        _fp(msg), _ip(row_ptr), _fp(base) if base is not None else None,
        _fp(out), n_rows, msg.shape[1], _stream()), "dm_seg_sum_f32")
    return out


def raw_seg_sum_gather(msg, perm, row_ptr, n_rows, base=None):
    _chk_f32(msg, base)
    out = torch.empty((n_rows,) + tuple(msg.shape[1:]), dtype=msg.dtype,
                      device=msg.device)
    _check(hip_lib().dm_seg_sum_gather_f32(
        _fp(msg), _ip(perm), _ip(row_ptr),
        _fp(base) if base is not None else None, _fp(out), n_rows,
        msg.shape[1], _stream()), "dm_seg_sum_gather_f32")
    return out


class _Gather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, perm, row_ptr):
        ctx.perm = perm          # None when idx is the sorted direction
        ctx.row_ptr = row_ptr
        ctx.n_rows = x.shape[0]
        return raw_gather(x, idx)

    @staticmethod
    def backward(ctx, grad):
        grad = grad.contiguous()
        if ctx.perm is None:
            gx = raw_seg_sum(grad, ctx.row_ptr, ctx.n_rows)
        else:
            gx = raw_seg_sum_gather(grad, ctx.perm, ctx.row_ptr, ctx.n_rows)
        return gx, None, None, None


def raw_silu_bwd(go_h, go_z, z):
    """dz = (go_z or 0) + go_h * silu'(z), one fused pass."""
    dz = torch.empty_like(z)
    _check(hip_lib().dm_silu_bwd_f32(
        _fp(go_h), _fp(go_z) if go_z is not None else None, _fp(z), _fp(dz),
        z.numel(), _stream()), "dm_silu_bwd_f32")
    return dz


ACT_CHECK_BLOCKS = 4096     # DM_ACT_CHECK_BLOCKS of distmlip_hip.h
ACT_SIGMOID, ACT_SILU = 0, 1


def raw_act_check(which: int, first_bits: int, count: int, device="cuda"):
    """Compares the kernels' sigmoid (which 0) or SiLU (1) with the plain
    expression 1/(1+expf(-x)) or x/(1+expf(-x)) on the count <= 2^32 fp32
    bit patterns from first_bits on.  Returns (mismatches, lowest mismatching
    pattern or None)."""
    bad = torch.empty(ACT_CHECK_BLOCKS, dtype=torch.int32, device=device)
    first = torch.empty(1, dtype=torch.int32, device=device)
    up = POINTER(ctypes.c_uint32)
    _check(hip_lib().dm_act_check_f32(
        which, first_bits, count, ctypes.cast(bad.data_ptr(), up),
        ctypes.cast(first.data_ptr(), up), _stream()), "dm_act_check_f32")
    n = int(bad.to(torch.int64).sum().item())
    return n, (first.item() & 0xffffffff) if n else None


def raw_act_eval(which: int, x: torch.Tensor, ref: bool) -> torch.Tensor:
    """sigmoid (which 0) or SiLU (1) of every element of x: the plain
    expression (ref) or the function the kernels call."""
    _chk_f32(x)
    out = torch.empty_like(x)
    _check(hip_lib().dm_act_eval_f32(
        which, 0 if ref else 1, _fp(x), x.numel(), _fp(out), _stream()),
        "dm_act_eval_f32")
    return out


class _GatherAdd3(torch.autograd.Function):
    """Emits (z, silu(z)) in one kernel; z doubles as the saved activation
    for the fused silu backward."""

    @staticmethod
    def forward(ctx, zs, zd, ze, src, dst, src_perm, src_row_ptr, row_ptr):
        _chk_f32(zs, zd, ze)
        # the z output is usually discarded (only h flows on): without this,
        # autograd materializes a full [E,2d] ZERO go_z every backward (a
        # zero-fill write + an extra read inside silu_bwd, ~0.8 ms/call at
        # li100k, rocprof run 17)
        ctx.set_materialize_grads(False)
        ctx.n_nodes = zs.shape[0]
        z = torch.empty_like(ze)
        # grad mode is always OFF inside Function.forward, so test the
        # inputs: when none requires grad (checkpoint outer pass /
        # inference) no backward will run and silu can go in place over z —
        # the kernel writes z then silu(z) per element, so a single buffer
        # is safe and halves the transient footprint
        if zs.requires_grad or zd.requires_grad or ze.requires_grad:
            h = torch.empty_like(ze)
        else:
            h = z
        _check(hip_lib().dm_gather_add3_f32(
            _fp(zs), _fp(zd), _fp(ze), _ip(src), _ip(dst), _fp(z), _fp(h),
            ze.shape[0], ze.shape[1], _stream()), "dm_gather_add3_f32")
        ctx.save_for_backward(src_perm, src_row_ptr, row_ptr, z)
        return z, h

    @staticmethod
    def backward(ctx, go_z, go_h):
        src_perm, src_row_ptr, row_ptr, z = ctx.saved_tensors
        if go_h is not None:
            dz = raw_silu_bwd(go_h.contiguous(),
                              go_z.contiguous() if go_z is not None else None,
                              z)
        else:
            dz = go_z.contiguous()
        gzs = raw_seg_sum_gather(dz, src_perm, src_row_ptr, ctx.n_nodes)
        gzd = raw_seg_sum(dz, row_ptr, ctx.n_nodes)
        return gzs, gzd, dz, None, None, None, None, None


def use_fused_mlp1_bwd() -> bool:
    """First-layer reverse kernel switch: DM_NO_FUSED_MLP1_BWD=1 restores
    the rocBLAS GEMM / addmm everywhere, for A/B runs in one build."""
    return os.environ.get("DM_NO_FUSED_MLP1_BWD", "0") != "1"


def raw_edge_mlp_bwd(dz, wt, gbase=None, out=None):
    """out = (gbase +) dz @ wt.t() in ONE kernel: the reverse of the fused
    first layer's per-edge GEMM, with the other gradient of the same rows
    added in its epilogue.  dz [E,128], wt [64,128] (the fusedT pack),
    gbase [E,64] or None.  out may be gbase (in place); only do that with a
    buffer the caller owns."""
    _chk_f32(dz, wt, gbase, out)
    E = dz.shape[0]
    assert dz.shape[1] == wt.shape[1]
    assert gbase is None or gbase.shape == (E, wt.shape[0])
    if out is None:
        out = torch.empty(E, wt.shape[0], dtype=dz.dtype, device=dz.device)
    assert out.shape == (E, wt.shape[0])
    _check(hip_lib().dm_edge_mlp_bwd_f32(
        _fp(dz), _fp(wt), _fp(gbase) if gbase is not None else None,
        _fp(out), E, dz.shape[1], wt.shape[0], _stream()),
        "dm_edge_mlp_bwd_f32")
    return out


def _first_layer_de(dz, wt):
    """dz @ wt.t(): dm_edge_mlp_bwd_f32 for the [64,128] pack, else (or
    with DM_NO_FUSED_MLP1_BWD=1) rocBLAS."""
    if (tuple(wt.shape) == (64, 128) and dz.dtype == torch.float32
            and use_fused_mlp1_bwd()):
        return raw_edge_mlp_bwd(dz, wt)
    return dz @ wt.t()


class _EdgeMlp3(torch.autograd.Function):
    """Fused first-layer edge MLP over the atom graph:
    (z, silu(z)) with z = erow @ WT + bias + zs[src] + zd[dst], the per-edge
    GEMM computed INSIDE the gather kernel (exact-fp32 MFMA tiles of 32
    edges per wave, WT staged in LDS) so the [E,2d] GEMM output is never
    materialized.  WT/bias must be frozen (inference
    path) — their grads are not produced."""

    @staticmethod
    def forward(ctx, erow, wt, bias, zs, zd, src, dst, src_perm, src_row_ptr,
                row_ptr):
        _chk_f32(erow, wt, bias, zs, zd)
        assert not wt.requires_grad and not bias.requires_grad
        ctx.set_materialize_grads(False)
        ctx.n_nodes = zs.shape[0]
        E, dout = erow.shape[0], wt.shape[1]
        h = torch.empty(E, dout, dtype=erow.dtype, device=erow.device)
        needs_z = erow.requires_grad or zs.requires_grad or zd.requires_grad
        z = torch.empty_like(h) if needs_z else h[:0]  # no bwd: skip z write
        _check(hip_lib().dm_edge_mlp3_f32(
            _fp(erow), _fp(wt), _fp(bias), _fp(zs), _fp(zd), _ip(src),
            _ip(dst), _fp(z) if needs_z else None, _fp(h), E, wt.shape[0],
            dout, _stream()), "dm_edge_mlp3_f32")
        ctx.save_for_backward(src_perm, src_row_ptr, row_ptr, z, wt)
        return z, h

    @staticmethod
    def backward(ctx, go_z, go_h):
        src_perm, src_row_ptr, row_ptr, z, wt = ctx.saved_tensors
        if go_h is not None:
            dz = raw_silu_bwd(go_h.contiguous(),
                              go_z.contiguous() if go_z is not None else None,
                              z)
        else:
            dz = go_z.contiguous()
        de = _first_layer_de(dz, wt)
        gzs = raw_seg_sum_gather(dz, src_perm, src_row_ptr, ctx.n_nodes)
        gzd = raw_seg_sum(dz, row_ptr, ctx.n_nodes)
        return de, None, None, gzs, gzd, None, None, None, None, None


class _EdgeMlp4(torch.autograd.Function):
    """Fused first-layer bond MLP over the line graph (3-gather form):
    z = arow @ WT + bias + z1[l_src] + z2[l_dst] + zv[center]."""

    @staticmethod
    def forward(ctx, arow, wt, bias, z1, z2, zv, pd):
        _chk_f32(arow, wt, bias, z1, z2, zv)
        assert not wt.requires_grad and not bias.requires_grad
        ctx.set_materialize_grads(False)
        ctx.pd = pd
        ctx.n_bonds = z1.shape[0]
        ctx.n_nodes = zv.shape[0]
        L, dout = arow.shape[0], wt.shape[1]
        h = torch.empty(L, dout, dtype=arow.dtype, device=arow.device)
        needs_z = (arow.requires_grad or z1.requires_grad or z2.requires_grad
                   or zv.requires_grad)
        z = torch.empty_like(h) if needs_z else h[:0]
        _check(hip_lib().dm_edge_mlp4_f32(
            _fp(arow), _fp(wt), _fp(bias), _fp(z1), _fp(z2), _fp(zv),
            _ip(pd.l_src), _ip(pd.l_dst), _ip(pd.center),
            _fp(z) if needs_z else None, _fp(h), L, wt.shape[0], dout,
            _stream()), "dm_edge_mlp4_f32")
        ctx.save_for_backward(z, wt)
        return z, h

    @staticmethod
    def backward(ctx, go_z, go_h):
        pd = ctx.pd
        z, wt = ctx.saved_tensors
        if go_h is not None:
            dz = raw_silu_bwd(go_h.contiguous(),
                              go_z.contiguous() if go_z is not None else None,
                              z)
        else:
            dz = go_z.contiguous()
        da = _first_layer_de(dz, wt)
        gz1 = raw_seg_sum_gather(dz, pd.line_src_perm, pd.line_src_row_ptr,
                                 ctx.n_bonds)
        gz2 = raw_seg_sum(dz, pd.line_row_ptr, ctx.n_bonds)
        gzv = raw_seg_sum_gather(dz, pd.center_perm, pd.center_row_ptr,
                                 ctx.n_nodes)
        return da, None, None, gz1, gz2, gzv, None


class _GatherAdd4(torch.autograd.Function):
    """Emits (z, silu(z)) over the line-graph 3-gather-add."""

    @staticmethod
    def forward(ctx, z1, z2, za, zv, pd):
        _chk_f32(z1, z2, za, zv)
        ctx.set_materialize_grads(False)   # see _GatherAdd3.forward
        ctx.pd = pd
        ctx.n_bonds = z1.shape[0]
        ctx.n_nodes = zv.shape[0]
        z = torch.empty_like(za)
        # see _GatherAdd3.forward: in-place silu only when no backward runs
        needs_h = (z1.requires_grad or z2.requires_grad or za.requires_grad
                   or zv.requires_grad)
        h = torch.empty_like(za) if needs_h else z
        _check(hip_lib().dm_gather_add4_f32(
            _fp(z1), _fp(z2), _fp(za), _fp(zv), _ip(pd.l_src), _ip(pd.l_dst),
            _ip(pd.center), _fp(z), _fp(h), za.shape[0], za.shape[1],
            _stream()), "dm_gather_add4_f32")
        ctx.save_for_backward(z)
        return z, h

    @staticmethod
    def backward(ctx, go_z, go_h):
        pd = ctx.pd
        (z,) = ctx.saved_tensors
        if go_h is not None:
            dz = raw_silu_bwd(go_h.contiguous(),
                              go_z.contiguous() if go_z is not None else None,
                              z)
        else:
            dz = go_z.contiguous()
        gz1 = raw_seg_sum_gather(dz, pd.line_src_perm, pd.line_src_row_ptr,
                                 ctx.n_bonds)
        gz2 = raw_seg_sum(dz, pd.line_row_ptr, ctx.n_bonds)
        gzv = raw_seg_sum_gather(dz, pd.center_perm, pd.center_row_ptr,
                                 ctx.n_nodes)
        return gz1, gz2, dz, gzv, None


class _SegSum(torch.autograd.Function):
    """out[n] = base[n] + sum of idx-sorted msg rows in [rp[n], rp[n+1])."""

    @staticmethod
    def forward(ctx, msg, idx, row_ptr, n_rows, base):
        ctx.save_for_backward(idx)
        ctx.has_base = base is not None
        return raw_seg_sum(msg.contiguous(), row_ptr, n_rows,
                           base.contiguous() if base is not None else None)

    @staticmethod
    def backward(ctx, grad):
        (idx,) = ctx.saved_tensors
        gmsg = raw_gather(grad.contiguous(), idx)
        gbase = grad if ctx.has_base else None
        return gmsg, None, None, None, gbase


class _GatedCombine(torch.autograd.Function):
    """out = base + silu(c) * sigmoid(g) * w — fused gated-MLP epilogue."""

    @staticmethod
    def forward(ctx, c, g, w, base):
        _chk_f32(c, g, w, base)
        ctx.save_for_backward(c, g) if w is None else \
            ctx.save_for_backward(c, g, w)
        ctx.has_w = w is not None
        ctx.has_base = base is not None
        out = torch.empty_like(c)
        _check(hip_lib().dm_gated_combine_fwd_f32(
            _fp(c), _fp(g), _fp(w) if w is not None else None,
            _fp(base) if base is not None else None, _fp(out), c.numel(),
            _stream()), "dm_gated_combine_fwd_f32")
        return out

    @staticmethod
    def backward(ctx, go):
        if ctx.has_w:
            c, g, w = ctx.saved_tensors
        else:
            c, g = ctx.saved_tensors
            w = None
        go = go.contiguous()
        dc = torch.empty_like(c)
        dg = torch.empty_like(g)
        dw = torch.empty_like(w) if ctx.has_w else None
        _check(hip_lib().dm_gated_combine_bwd_f32(
            _fp(go), _fp(c), _fp(g), _fp(w) if w is not None else None,
            _fp(dc), _fp(dg), _fp(dw) if dw is not None else None,
            c.numel(), _stream()), "dm_gated_combine_bwd_f32")
        return dc, dg, dw, (go if ctx.has_base else None)


class _EdgeGeomRbf(torch.autograd.Function):
    """Fused bond_vec/bond_dist/RBF*envelope (chgnet.py:96-124 analog)."""

    @staticmethod
    def forward(ctx, pos, offshift, freqs, cutoff, pexp, pd):
        _chk_f32(pos, offshift, freqs)
        E = offshift.shape[0]
        nrbf = freqs.shape[0]
        bv = torch.empty(E, 3, dtype=pos.dtype, device=pos.device)
        bd = torch.empty(E, dtype=pos.dtype, device=pos.device)
        exp_out = torch.empty(E, nrbf, dtype=pos.dtype, device=pos.device)
        _check(hip_lib().dm_edge_geom_rbf_fwd_f32(
            _fp(pos), _ip(pd.src), _ip(pd.dst), _fp(offshift), _fp(freqs),
            float(cutoff), int(pexp), nrbf, _fp(bv), _fp(bd), _fp(exp_out),
            E, _stream()), "dm_edge_geom_rbf_fwd_f32")
        ctx.save_for_backward(bv, bd, freqs)
        ctx.set_materialize_grads(False)   # bv/bd grads are often absent
        ctx.pd = pd
        ctx.cutoff, ctx.pexp, ctx.nrbf = float(cutoff), int(pexp), nrbf
        ctx.n_nodes = pos.shape[0]
        return bv, bd, exp_out

    @staticmethod
    def backward(ctx, go_bv, go_bd, go_exp):
        bv, bd, freqs = ctx.saved_tensors
        pd = ctx.pd
        E = bv.shape[0]
        gbv = torch.empty_like(bv)
        go_exp = go_exp.contiguous() if go_exp is not None else \
            torch.zeros(E, ctx.nrbf, dtype=bv.dtype, device=bv.device)
        _check(hip_lib().dm_edge_geom_rbf_bwd_f32(
            _fp(go_bv.contiguous()) if go_bv is not None else None,
            _fp(go_bd.contiguous()) if go_bd is not None else None,
            _fp(go_exp), _fp(bv), _fp(bd), _fp(freqs), ctx.cutoff, ctx.pexp,
            ctx.nrbf, _fp(gbv), E, _stream()), "dm_edge_geom_rbf_bwd_f32")
        g_pos = raw_seg_sum(gbv, pd.row_ptr, ctx.n_nodes) - \
            raw_seg_sum_gather(gbv, pd.src_perm, pd.src_row_ptr, ctx.n_nodes)
        # freqs gradient not implemented (inference engine; forces only)
        return g_pos, gbv, None, None, None, None


class _RbfEnv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d, freqs, cutoff, pexp):
        _chk_f32(d, freqs)
        M, nrbf = d.shape[0], freqs.shape[0]
        out = torch.empty(M, nrbf, dtype=d.dtype, device=d.device)
        _check(hip_lib().dm_rbf_env_fwd_f32(
            _fp(d), _fp(freqs), float(cutoff), int(pexp), nrbf, _fp(out), M,
            _stream()), "dm_rbf_env_fwd_f32")
        ctx.save_for_backward(d, freqs)
        ctx.cutoff, ctx.pexp, ctx.nrbf = float(cutoff), int(pexp), nrbf
        return out

    @staticmethod
    def backward(ctx, go):
        d, freqs = ctx.saved_tensors
        gd = torch.empty_like(d)
        _check(hip_lib().dm_rbf_env_bwd_f32(
            _fp(go.contiguous()), _fp(d), _fp(freqs), ctx.cutoff, ctx.pexp,
            ctx.nrbf, _fp(gd), d.shape[0], _stream()), "dm_rbf_env_bwd_f32")
        return gd, None, None, None


class _GatedCombinePacked(torch.autograd.Function):
    """gated_combine over PACKED cg [2,E,D] (cg[0]=c, cg[1]=g): avoids the
    h-slice / c-g-select gradient zero+copy+add passes entirely."""

    @staticmethod
    def forward(ctx, cg, w, base):
        _chk_f32(cg, w, base)
        half = cg.shape[1] * cg.shape[2]
        c_ptr = ctypes.cast(cg.data_ptr(), POINTER(c_float))
        g_ptr = ctypes.cast(cg.data_ptr() + 4 * half, POINTER(c_float))
        out = torch.empty(cg.shape[1], cg.shape[2], dtype=cg.dtype,
                          device=cg.device)
        _check(hip_lib().dm_gated_combine_fwd_f32(
            c_ptr, g_ptr, _fp(w) if w is not None else None,
            _fp(base) if base is not None else None, _fp(out), half,
            _stream()), "dm_gated_combine_fwd_f32")
        ctx.save_for_backward(cg, w) if w is not None else             ctx.save_for_backward(cg)
        ctx.has_w = w is not None
        ctx.has_base = base is not None
        return out

    @staticmethod
    def backward(ctx, go):
        if ctx.has_w:
            cg, w = ctx.saved_tensors
        else:
            (cg,) = ctx.saved_tensors
            w = None
        go = go.contiguous()
        half = cg.shape[1] * cg.shape[2]
        dcg = torch.empty_like(cg)
        c_ptr = ctypes.cast(cg.data_ptr(), POINTER(c_float))
        g_ptr = ctypes.cast(cg.data_ptr() + 4 * half, POINTER(c_float))
        dc_ptr = ctypes.cast(dcg.data_ptr(), POINTER(c_float))
        dg_ptr = ctypes.cast(dcg.data_ptr() + 4 * half, POINTER(c_float))
        dw = torch.empty_like(w) if ctx.has_w else None
        _check(hip_lib().dm_gated_combine_bwd_f32(
            _fp(go), c_ptr, g_ptr, _fp(w) if w is not None else None,
            dc_ptr, dg_ptr, _fp(dw) if dw is not None else None, half,
            _stream()), "dm_gated_combine_bwd_f32")
        return dcg, dw, (go if ctx.has_base else None)


class RadialW:
    """A shared message weight in factored form, accepted wherever
    HipOps.mlp_tail_act, r_mlp_tail_fwd, r_gated_mlp3 and r_mlp_tail_bwd take
    a dense w [E,d]:
        w = (bexp @ W.t()) * mask
    with bexp [E,n_rbf], W [d,n_rbf] and mask [E] (or [E,1]) or None.  The
    kernels compute w where they use it (one fixed fp32 order, the same bits
    in all of them) and the dense array never exists.  r_mlp_tail_bwd then
    returns (dz, dbexp) instead of (dz, dw), with dbexp = (dw * mask) @ W
    added onto dbexp_acc in place when that is given."""

    __slots__ = ("bexp", "W", "mask", "dbexp_acc")

    def __init__(self, bexp, W, mask=None, dbexp_acc=None):
        self.bexp, self.W, self.dbexp_acc = bexp, W, dbexp_acc
        self.mask = mask.reshape(-1) if mask is not None else None

    @property
    def requires_grad(self):
        return self.bexp.requires_grad

    def with_acc(self, dbexp_acc):
        return RadialW(self.bexp, self.W, self.mask, dbexp_acc)

    def check(self, E, d):
        _chk_f32(self.bexp, self.W, self.mask, self.dbexp_acc)
        assert self.bexp.shape[0] == E and self.W.shape == (
            d, self.bexp.shape[1])
        assert self.mask is None or self.mask.shape == (E,)
        assert self.dbexp_acc is None \
            or self.dbexp_acc.shape == self.bexp.shape

    def ptrs(self):
        return (_fp(self.bexp), _fp(self.W),
                _fp(self.mask) if self.mask is not None else None)


def use_factored_w() -> bool:
    """Factored message weights switch: DM_NO_FACTORED_W=1 restores the dense
    [E,d] weights (bexp @ W.t() by rocBLAS) everywhere, for A/B runs in one
    build."""
    return os.environ.get("DM_NO_FACTORED_W", "0") != "1"


def _raw_mlp_tail_bwd_fw(go, cg, rw, z, w2, go_idx):
    """raw_mlp_tail_bwd with a RadialW: (dz, dbexp)."""
    _chk_f32(go, cg, z, w2)
    d = go.shape[1]
    E = go.shape[0] if go_idx is None else go_idx.shape[0]
    assert cg.shape == (2, E, d) and z.shape == (E, 2 * d)
    assert w2.shape == (2, d, d)
    rw.check(E, d)
    if go_idx is not None:
        assert go_idx.dtype == torch.int32 and go_idx.is_contiguous() \
            and go_idx.device == go.device
    half = E * d
    dz = torch.empty_like(z)
    acc = rw.dbexp_acc
    dbexp = acc if acc is not None else torch.empty_like(rw.bexp)
    bexp_p, W_p, mask_p = rw.ptrs()
    _check(hip_lib().dm_gated_mlp_tail_bwd_fw_f32(
        _fp(go), _ip(go_idx) if go_idx is not None else None,
        ctypes.cast(cg.data_ptr(), POINTER(c_float)),
        ctypes.cast(cg.data_ptr() + 4 * half, POINTER(c_float)),
        bexp_p, W_p, mask_p, _fp(z),
        ctypes.cast(w2.data_ptr(), POINTER(c_float)),
        ctypes.cast(w2.data_ptr() + 4 * d * d, POINTER(c_float)),
        _fp(dz), _fp(acc) if acc is not None else None, _fp(dbexp), E, d,
        rw.bexp.shape[1], _stream()), "dm_gated_mlp_tail_bwd_fw_f32")
    return dz, dbexp


def raw_mlp_tail_bwd(go, cg, w, z, w2, go_idx=None):
    """(dz, dw) of one gated MLP's tail in ONE kernel: the reverse of
    out = base + silu(cg[0]) * sigmoid(cg[1]) * w with cg = the second layer
    over silu(z).  go [E,d], cg [2,E,d] packed, w [E,d] or None, z [E,2d],
    w2 [2,d,d] (input x output per half).  d must be 64.  With go_idx
    (int32 [E]) go is a [N,d] table and row r takes go[go_idx[r]]: the
    result on the materialized go[go_idx], without that gather.
    w may be a RadialW: (dz, dbexp) is returned then."""
    if isinstance(w, RadialW):
        return _raw_mlp_tail_bwd_fw(go, cg, w, z, w2, go_idx)
    _chk_f32(go, cg, w, z, w2)
    d = go.shape[1]
    E = go.shape[0] if go_idx is None else go_idx.shape[0]
    assert cg.shape == (2, E, d) and z.shape == (E, 2 * d)
    assert w2.shape == (2, d, d) and (w is None or w.shape == (E, d))
    half = E * d
    dz = torch.empty_like(z)
    dw = torch.empty_like(w) if w is not None else None
    if go_idx is not None:
        assert go_idx.dtype == torch.int32 and go_idx.is_contiguous() \
            and go_idx.device == go.device
        _check(hip_lib().dm_gated_mlp_tail_bwd_idx_f32(
            _fp(go), _ip(go_idx),
            ctypes.cast(cg.data_ptr(), POINTER(c_float)),
            ctypes.cast(cg.data_ptr() + 4 * half, POINTER(c_float)),
            _fp(w) if w is not None else None, _fp(z),
            ctypes.cast(w2.data_ptr(), POINTER(c_float)),
            ctypes.cast(w2.data_ptr() + 4 * d * d, POINTER(c_float)),
            _fp(dz), _fp(dw) if dw is not None else None, E, d, _stream()),
            "dm_gated_mlp_tail_bwd_idx_f32")
        return dz, dw
    _check(hip_lib().dm_gated_mlp_tail_bwd_f32(
        _fp(go), ctypes.cast(cg.data_ptr(), POINTER(c_float)),
        ctypes.cast(cg.data_ptr() + 4 * half, POINTER(c_float)),
        _fp(w) if w is not None else None, _fp(z),
        ctypes.cast(w2.data_ptr(), POINTER(c_float)),
        ctypes.cast(w2.data_ptr() + 4 * d * d, POINTER(c_float)),
        _fp(dz), _fp(dw) if dw is not None else None, E, d, _stream()),
        "dm_gated_mlp_tail_bwd_f32")
    return dz, dw


def use_fused_tail_fwd() -> bool:
    """Forward-tail kernel switch: DM_NO_FUSED_MLP_FWD=1 restores baddbmm +
    dm_gated_combine_fwd_f32 everywhere, for A/B runs in one build."""
    return os.environ.get("DM_NO_FUSED_MLP_FWD", "0") != "1"


def raw_mlp_tail_fwd(h, w2, b2, w, base, keep_cg):
    """(out, cg or None) of one gated MLP's tail in ONE kernel:
    cg = baddbmm(b2, h halves, w2) and out = base + silu(cg[0]) *
    sigmoid(cg[1]) * w.  h [E,2d], w2 [2,d,d] (input x output per half),
    b2 [2,1,d], w and base [E,d] or None.  cg [2,E,d] packed is written and
    returned only with keep_cg; out is the same bit for bit either way.
    d must be 64.  w may be a RadialW."""
    rw = w if isinstance(w, RadialW) else None
    if rw is not None:
        w = None
    _chk_f32(h, w2, b2, w, base)
    E, d = h.shape[0], w2.shape[1]
    assert h.shape == (E, 2 * d) and w2.shape == (2, d, d)
    assert b2.numel() == 2 * d
    assert w is None or w.shape == (E, d)
    assert base is None or base.shape == (E, d)
    half = E * d
    out = torch.empty(E, d, dtype=h.dtype, device=h.device)
    cg = torch.empty(2, E, d, dtype=h.dtype, device=h.device) \
        if keep_cg else None
    if rw is not None:
        rw.check(E, d)
        _check(hip_lib().dm_gated_mlp_tail_fwd_fw_f32(
            _fp(h), ctypes.cast(w2.data_ptr(), POINTER(c_float)),
            ctypes.cast(w2.data_ptr() + 4 * d * d, POINTER(c_float)),
            ctypes.cast(b2.data_ptr(), POINTER(c_float)),
            ctypes.cast(b2.data_ptr() + 4 * d, POINTER(c_float)),
            *rw.ptrs(), _fp(base) if base is not None else None,
            ctypes.cast(cg.data_ptr(), POINTER(c_float)) if keep_cg else None,
            ctypes.cast(cg.data_ptr() + 4 * half, POINTER(c_float))
            if keep_cg else None,
            _fp(out), E, d, rw.bexp.shape[1], _stream()),
            "dm_gated_mlp_tail_fwd_fw_f32")
        return out, cg
    _check(hip_lib().dm_gated_mlp_tail_fwd_f32(
        _fp(h), ctypes.cast(w2.data_ptr(), POINTER(c_float)),
        ctypes.cast(w2.data_ptr() + 4 * d * d, POINTER(c_float)),
        ctypes.cast(b2.data_ptr(), POINTER(c_float)),
        ctypes.cast(b2.data_ptr() + 4 * d, POINTER(c_float)),
        _fp(w) if w is not None else None,
        _fp(base) if base is not None else None,
        ctypes.cast(cg.data_ptr(), POINTER(c_float)) if keep_cg else None,
        ctypes.cast(cg.data_ptr() + 4 * half, POINTER(c_float))
        if keep_cg else None,
        _fp(out), E, d, _stream()), "dm_gated_mlp_tail_fwd_f32")
    return out, cg


def use_fused_mlp_full() -> bool:
    """Whole-MLP kernel switch: DM_NO_FUSED_MLP_FULL=1 restores the
    first-layer + tail kernel pair everywhere, for A/B runs in one build."""
    return os.environ.get("DM_NO_FUSED_MLP_FULL", "0") != "1"


def raw_gated_mlp(row, wt, bias, tables, idx, w2, b2, w, base, keep,
                  want_out=True):
    """One whole gated MLP in ONE kernel (dm_gated_mlp3/4_f32): the fused
    first layer over row [E,64] and 2 or 3 gathered tables, the second layer
    and the combine, without the h [E,128] array between them.  Returns
    (z, cg, out): z [E,128] and cg [2,E,64] packed with keep, else None; out
    None with want_out=False (keep only; w and base are then not read).
    Values are the two-kernel path's bit for bit.  w may be a RadialW (two
    tables, with out)."""
    rw = w if isinstance(w, RadialW) and want_out else None
    if isinstance(w, RadialW):
        w = None
    _chk_f32(row, wt, bias, *tables, w2, b2, w, base)
    E, d = row.shape[0], w2.shape[1]
    assert wt.shape == (d, 2 * d) and w2.shape == (2, d, d)
    assert b2.numel() == 2 * d and bias.numel() == 2 * d
    assert len(tables) == len(idx) and len(tables) in (2, 3)
    assert all(t.shape[1] == 2 * d for t in tables)
    assert keep or want_out
    if not want_out:
        w = base = None
    assert w is None or w.shape == (E, d)
    assert base is None or base.shape == (E, d)
    half = E * d
    z = torch.empty(E, 2 * d, dtype=row.dtype, device=row.device) \
        if keep else None
    if E == 0:
        e0 = row.new_empty
        return z, e0(2, 0, d) if keep else None, e0(0, d) if want_out else None
    cg = torch.empty(2, E, d, dtype=row.dtype, device=row.device) \
        if keep else None
    out = torch.empty(E, d, dtype=row.dtype, device=row.device) \
        if want_out else None

    def at(t, off=0):
        return ctypes.cast(t.data_ptr() + off, POINTER(c_float))
    tail = (at(w2), at(w2, 4 * d * d), at(b2), at(b2, 4 * d),
            _fp(w) if w is not None else None,
            _fp(base) if base is not None else None,
            _fp(z) if keep else None,
            at(cg) if keep else None, at(cg, 4 * half) if keep else None,
            _fp(out) if want_out else None, E, wt.shape[0], d, _stream())
    if rw is not None:
        assert len(tables) == 2, "a factored w takes the two-gather form"
        rw.check(E, d)
        tail = tail[:4] + rw.ptrs() + tail[5:-1] + (rw.bexp.shape[1],
                                                    _stream())
        _check(hip_lib().dm_gated_mlp3_fw_f32(
            _fp(row), _fp(wt), _fp(bias), _fp(tables[0]), _fp(tables[1]),
            _ip(idx[0]), _ip(idx[1]), *tail), "dm_gated_mlp3_fw_f32")
        return z, cg, out
    if len(tables) == 2:
        _check(hip_lib().dm_gated_mlp3_f32(
            _fp(row), _fp(wt), _fp(bias), _fp(tables[0]), _fp(tables[1]),
            _ip(idx[0]), _ip(idx[1]), *tail), "dm_gated_mlp3_f32")
    else:
        _check(hip_lib().dm_gated_mlp4_f32(
            _fp(row), _fp(wt), _fp(bias), _fp(tables[0]), _fp(tables[1]),
            _fp(tables[2]), _ip(idx[0]), _ip(idx[1]), _ip(idx[2]), *tail),
            "dm_gated_mlp4_f32")
    return z, cg, out


def _no_grad_inputs(*ts):
    return not (torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in ts))


def _cont(t):
    return t.contiguous() if t is not None else None


class _GatedMlpTail(torch.autograd.Function):
    """Everything of a gated MLP after its first layer, as one node:
    out = base + silu(c) * sigmoid(g) * w with cg = baddbmm(b2, h halves,
    w2).  The forward is the single dm_gated_mlp_tail_fwd_f32 launch, which
    writes cg for the backward and never reads it back (with
    DM_NO_FUSED_MLP_FWD=1: the baddbmm and dm_gated_combine_fwd_f32 of
    chgnet._SecondLayer + _GatedCombinePacked); the backward is the single
    dm_gated_mlp_tail_bwd_f32 launch, which goes from go to dz without
    writing dcg or dh.

    Contract: z and h are the two outputs of ONE first-layer call
    (_EdgeMlp3/4, _GatherAdd3/4), so h == silu(z).  The gradient is then
    returned on z (dz = dh * silu'(z)) and None on h; the producer's
    backward takes go_z as dz when go_h is None.  Passing an h that is not
    silu(z) of the given z gives wrong gradients: HipOps.mlp_tail checks
    that both come from the same autograd node.  w2/b2 are frozen packs
    (no weight grads)."""

    @staticmethod
    def forward(ctx, z, h, w2, b2, w, base):
        _chk_f32(z, h, w2, w, base)
        d = w2.shape[1]
        assert z.shape == h.shape and z.shape[1] == 2 * d
        assert not w2.requires_grad and not b2.requires_grad
        if d == 64 and use_fused_tail_fwd():
            out, cg = raw_mlp_tail_fwd(h, w2, b2, w, base, True)
        else:
            cg = torch.baddbmm(b2, h.view(-1, 2, d).transpose(0, 1), w2)
            half = cg.shape[1] * d
            out = torch.empty(cg.shape[1], d, dtype=cg.dtype,
                              device=cg.device)
            _check(hip_lib().dm_gated_combine_fwd_f32(
                ctypes.cast(cg.data_ptr(), POINTER(c_float)),
                ctypes.cast(cg.data_ptr() + 4 * half, POINTER(c_float)),
                _fp(w) if w is not None else None,
                _fp(base) if base is not None else None, _fp(out), half,
                _stream()), "dm_gated_combine_fwd_f32")
        ctx.save_for_backward(cg, z, w2, w)
        ctx.has_base = base is not None
        return out

    @staticmethod
    def backward(ctx, go):
        cg, z, w2, w = ctx.saved_tensors
        go = go.contiguous()
        dz, dw = raw_mlp_tail_bwd(go, cg, w, z, w2)
        return dz, None, None, None, dw, (go if ctx.has_base else None)


class HipOps:
    """Product ops backend (see ops_base.OpsBackend)."""

    is_reference = False
    tail_bwd_indexed = True      # r_mlp_tail_bwd takes go_idx
    factored_w = True            # the w of the MLP tails may be a RadialW

    def gather(self, x, idx, csr=None):
        if csr is None:
            raise RuntimeError("HipOps.gather needs a (perm, row_ptr) CSR "
                               "for its deterministic backward")
        return _Gather.apply(x.contiguous(), idx, csr[0], csr[1])

    # The *_zh forms return (z, silu(z)) of one first-layer call, the pair
    # mlp_tail takes; the *_act forms return silu(z) alone.

    def gather_add3_zh(self, zs, zd, ze, pd):
        return _GatherAdd3.apply(zs.contiguous(), zd.contiguous(),
                                 ze.contiguous(), pd.src, pd.dst,
                                 pd.src_perm, pd.src_row_ptr, pd.row_ptr)

    def gather_add3_act(self, zs, zd, ze, pd):
        """silu(zs[src] + zd[dst] + ze), silu fused into the gather kernel."""
        return self.gather_add3_zh(zs, zd, ze, pd)[1]

    def edge_mlp3_zh(self, erow, wt, bias, zs, zd, pd):
        return _EdgeMlp3.apply(erow.contiguous(), wt, bias, zs.contiguous(),
                               zd.contiguous(), pd.src, pd.dst, pd.src_perm,
                               pd.src_row_ptr, pd.row_ptr)

    def edge_mlp3_act(self, erow, wt, bias, zs, zd, pd):
        """silu(erow @ wt + bias + zs[src] + zd[dst]) fused in one kernel
        (wt = first-layer weight.T, [64,128] only)."""
        return self.edge_mlp3_zh(erow, wt, bias, zs, zd, pd)[1]

    def edge_mlp4_zh(self, arow, wt, bias, z1, z2, zv, pd):
        return _EdgeMlp4.apply(arow.contiguous(), wt, bias, z1.contiguous(),
                               z2.contiguous(), zv.contiguous(), pd)

    def edge_mlp4_act(self, arow, wt, bias, z1, z2, zv, pd):
        return self.edge_mlp4_zh(arow, wt, bias, z1, z2, zv, pd)[1]

    def gather_add4_zh(self, z1, z2, za, zv, pd):
        return _GatherAdd4.apply(z1.contiguous(), z2.contiguous(),
                                 za.contiguous(), zv.contiguous(), pd)

    def gather_add4_act(self, z1, z2, za, zv, pd):
        return self.gather_add4_zh(z1, z2, za, zv, pd)[1]

    def mlp_tail(self, z, h, w2, b2, w=None, base=None):
        """base + silu(c) * sigmoid(g) * w over cg = second layer of h, with
        the one-kernel reverse pass (_GatedMlpTail).  (z, h) must be the
        pair returned by ONE *_zh call of a grad-recording pass."""
        assert z.grad_fn is not None and z.grad_fn is h.grad_fn, \
            "mlp_tail: z and h must be the outputs of one first-layer call"
        assert z.shape == h.shape and w2.shape[1] * 2 == z.shape[1]
        return _GatedMlpTail.apply(
            z, h, w2, b2, w.contiguous() if w is not None else None,
            base.contiguous() if base is not None else None)

    def mlp_tail_act(self, h, w2, b2, w=None, base=None):
        """mlp_tail's value for passes that record nothing (torch.no_grad
        inference, the lean recompute forwards of conv.py): out only, no cg is
        allocated or written.  Not differentiable: refused when an input
        would need a gradient."""
        assert not (torch.is_grad_enabled() and any(
            t is not None and t.requires_grad for t in (h, w, base))), \
            "mlp_tail_act is the no-grad form; use mlp_tail"
        if not isinstance(w, RadialW):
            w = w.contiguous() if w is not None else None
        return raw_mlp_tail_fwd(
            h.contiguous(), w2, b2, w,
            base.contiguous() if base is not None else None, False)[0]

    def scatter_edges(self, msg, pd, base=None):
        return _SegSum.apply(msg, pd.dst, pd.row_ptr, pd.n_atoms, base)

    def scatter_rows(self, msg, dst_rel, row_ptr_rel, n_rows):
        """Segment-sum of dst-sorted msg rows over an arbitrary local CSR
        (node-range-chunked message passes; dst_rel/row_ptr_rel are
        relative to the range start)."""
        return _SegSum.apply(msg, dst_rel, row_ptr_rel, n_rows, None)

    # -- raw (non-differentiable) primitives for the hand-sequenced conv
    #    backward (distmlip_amd.conv); see ops_base docstring ------------

    def r_gather_add3(self, zs, zd, ze, pd):
        _chk_f32(zs, zd, ze)
        z = torch.empty_like(ze)
        h = torch.empty_like(ze)
        _check(hip_lib().dm_gather_add3_f32(
            _fp(zs), _fp(zd), _fp(ze), _ip(pd.src), _ip(pd.dst), _fp(z),
            _fp(h), ze.shape[0], ze.shape[1], _stream()),
            "dm_gather_add3_f32")
        return z, h

    def _cg_ptrs(self, cg):
        half = cg.shape[1] * cg.shape[2]
        return (ctypes.cast(cg.data_ptr(), POINTER(c_float)),
                ctypes.cast(cg.data_ptr() + 4 * half, POINTER(c_float)),
                half)

    def r_combine_fwd(self, cg, w, base):
        _chk_f32(cg, w, base)
        c_ptr, g_ptr, half = self._cg_ptrs(cg)
        out = torch.empty(cg.shape[1], cg.shape[2], dtype=cg.dtype,
                          device=cg.device)
        _check(hip_lib().dm_gated_combine_fwd_f32(
            c_ptr, g_ptr, _fp(w) if w is not None else None,
            _fp(base) if base is not None else None, _fp(out), half,
            _stream()), "dm_gated_combine_fwd_f32")
        return out

    def r_combine_bwd(self, go, cg, w):
        _chk_f32(go, cg, w)
        c_ptr, g_ptr, half = self._cg_ptrs(cg)
        dcg = torch.empty_like(cg)
        dc_ptr = ctypes.cast(dcg.data_ptr(), POINTER(c_float))
        dg_ptr = ctypes.cast(dcg.data_ptr() + 4 * half, POINTER(c_float))
        dw = torch.empty_like(w) if w is not None else None
        _check(hip_lib().dm_gated_combine_bwd_f32(
            _fp(go), c_ptr, g_ptr, _fp(w) if w is not None else None,
            dc_ptr, dg_ptr, _fp(dw) if dw is not None else None, half,
            _stream()), "dm_gated_combine_bwd_f32")
        return dcg, dw

    def r_silu_bwd(self, go_h, z):
        return raw_silu_bwd(go_h.contiguous(), None, z)

    def r_mlp_tail_bwd(self, go, cg, w, z, w2, go_idx=None):
        """(dz, dw): r_combine_bwd + second-layer reverse + r_silu_bwd in
        one kernel (d = 64 only).  go_idx: go is a node table read by index
        (r_gather_dst folded in).  With w a RadialW: (dz, dbexp)."""
        return raw_mlp_tail_bwd(go, cg, w, z, w2, go_idx)

    def r_edge_mlp3(self, erow, wt, bias, zs, zd, pd):
        """(z, h) of the fused first layer with z stored: r_gather_add3
        over addmm(bias, erow, wt) without that [E,2d] transient (wt =
        the [64,128] fusedT pack only)."""
        _chk_f32(erow, wt, bias, zs, zd)
        E, dout = erow.shape[0], wt.shape[1]
        z = torch.empty(E, dout, dtype=erow.dtype, device=erow.device)
        h = torch.empty_like(z)
        _check(hip_lib().dm_edge_mlp3_f32(
            _fp(erow), _fp(wt), _fp(bias), _fp(zs), _fp(zd), _ip(pd.src),
            _ip(pd.dst), _fp(z), _fp(h), E, wt.shape[0], dout, _stream()),
            "dm_edge_mlp3_f32")
        return z, h

    def r_edge_mlp_bwd(self, dz, wt, gbase=None, out=None):
        """(gbase +) dz @ wt.t() in one kernel (wt = the [64,128] fusedT
        pack only); out may be gbase when the caller owns it."""
        return raw_edge_mlp_bwd(dz, wt, gbase, out)

    def r_move_rows(self, src, si, dst, di, add=False):
        """dst[di] (=|+=) src[si] by rows, in place over dst, one kernel;
        si / di int64 or None (identity), di unique."""
        return raw_move_rows(src, si, dst, di, add)

    def r_zero_rows(self, dst, di):
        """dst[di] = 0 by rows, in place, one kernel."""
        return raw_zero_rows(dst, di)

    def r_mlp_tail_fwd(self, h, w2, b2, w, base):
        """(cg, out): second layer + r_combine_fwd in one kernel (d = 64
        only)."""
        out, cg = raw_mlp_tail_fwd(h, w2, b2, w, base, True)
        return cg, out

    # whole gated MLP in one kernel (first layer, second layer, combine)

    def gated_mlp4_act(self, arow, wt, bias, z1, z2, zv, pd, w2, b2, w=None,
                       base=None):
        """mlp_tail_act(edge_mlp4_act(...), w2, b2, w, base) in one kernel,
        h never reaching memory; for passes that record nothing."""
        assert _no_grad_inputs(arow, z1, z2, zv, w, base), \
            "gated_mlp4_act is the no-grad form"
        return raw_gated_mlp(arow.contiguous(), wt, bias,
                             (z1.contiguous(), z2.contiguous(),
                              zv.contiguous()),
                             (pd.l_src, pd.l_dst, pd.center), w2, b2,
                             _cont(w), _cont(base), False)[2]

    def r_gated_mlp3(self, erow, wt, bias, zs, zd, pd, w2, b2, w, base,
                     want_out=True):
        """(z, cg, out) of r_edge_mlp3 + r_mlp_tail_fwd in one kernel; out
        is None with want_out=False, and w and base are then not read."""
        return raw_gated_mlp(erow, wt, bias, (zs, zd), (pd.src, pd.dst), w2,
                             b2, w, base, True, want_out)

    def r_gather_dst(self, x, pd):
        return raw_gather(x.contiguous(), pd.dst)

    def r_seg_dst(self, msg, pd, base=None):
        return raw_seg_sum(msg, pd.row_ptr, pd.n_atoms, base)

    def r_seg_src(self, msg, pd):
        return raw_seg_sum_gather(msg, pd.src_perm, pd.src_row_ptr,
                                  pd.n_atoms)

    # line-graph raw primitives (bond-conv hand-sequenced reverse)

    def r_gather_add4(self, z1, z2, za, zv, pd):
        _chk_f32(z1, z2, za, zv)
        z = torch.empty_like(za)
        h = torch.empty_like(za)
        _check(hip_lib().dm_gather_add4_f32(
            _fp(z1), _fp(z2), _fp(za), _fp(zv), _ip(pd.l_src), _ip(pd.l_dst),
            _ip(pd.center), _fp(z), _fp(h), za.shape[0], za.shape[1],
            _stream()), "dm_gather_add4_f32")
        return z, h

    def r_gather_lsrc(self, x, pd):
        return raw_gather(x.contiguous(), pd.l_src)

    def r_gather_ldst(self, x, pd):
        return raw_gather(x.contiguous(), pd.l_dst)

    def r_seg_ldst(self, msg, pd, base=None):
        return raw_seg_sum(msg, pd.line_row_ptr, pd.n_bonds, base)

    def r_seg_lsrc(self, msg, pd):
        return raw_seg_sum_gather(msg, pd.line_src_perm, pd.line_src_row_ptr,
                                  pd.n_bonds)

    def r_seg_center(self, msg, pd):
        return raw_seg_sum_gather(msg, pd.center_perm, pd.center_row_ptr,
                                  pd.n_atoms)

    def scatter_lines(self, msg, pd, base=None):
        return _SegSum.apply(msg, pd.l_dst, pd.line_row_ptr, pd.n_bonds, base)

    def gated_combine(self, c, g, w=None, base=None):
        return _GatedCombine.apply(
            c.contiguous(), g.contiguous(),
            w.contiguous() if w is not None else None,
            base.contiguous() if base is not None else None)

    def gated_combine_packed(self, cg, w=None, base=None):
        return _GatedCombinePacked.apply(
            cg.contiguous(),
            w.contiguous() if w is not None else None,
            base.contiguous() if base is not None else None)

    def edge_geom_rbf(self, pos, offshift, freqs, cutoff, pexp, pd):
        return _EdgeGeomRbf.apply(pos.contiguous(), offshift.contiguous(),
                                  freqs.contiguous(), cutoff, pexp, pd)

    def rbf_env(self, d, freqs, cutoff, pexp):
        return _RbfEnv.apply(d.contiguous(), freqs.contiguous(), cutoff, pexp)
