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
from ctypes import POINTER, c_char_p, c_float, c_int32, c_int64, c_uint64

import torch

from distmlip_amd import mlp_path
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
        lib.dm_edge_mlp_bwd_patch_f32.restype = c_int32
        lib.dm_edge_mlp_bwd_patch_f32.argtypes = [fp, fp, fp, ip, fp, fp,
                                                  c_int64, c_int64, c_int64,
                                                  c_uint64]
        lib.dm_edge_mlp_bwd_src_f32.restype = c_int32
        lib.dm_edge_mlp_bwd_src_f32.argtypes = [
            fp, fp, fp, ip, fp, fp, ip, ip, ip, fp, POINTER(ctypes.c_double),
            c_int64, c_int64, c_int64, c_int64, c_uint64]
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
        # the reverse tail with the dst segment sums of dz in its epilogue
        lib.dm_gated_mlp_tail_bwd_seg_f32.restype = c_int32
        lib.dm_gated_mlp_tail_bwd_seg_f32.argtypes = [
            fp, ip, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, ip,
            ip, fp, POINTER(ctypes.c_double), c_int64, c_int64, c_int64,
            c_int64, c_uint64]
        # dense w read through a row index (w_idx)
        lib.dm_gated_mlp_tail_fwd_widx_f32.restype = c_int32
        lib.dm_gated_mlp_tail_fwd_widx_f32.argtypes = [
            fp, fp, fp, fp, fp, fp, ip, fp, fp, fp, fp, c_int64, c_int64,
            c_uint64]
        lib.dm_gated_mlp4_widx_f32.restype = c_int32
        lib.dm_gated_mlp4_widx_f32.argtypes = [
            fp, fp, fp, fp, fp, fp, ip, ip, ip, fp, fp, fp, fp, fp, ip, fp, fp,
            fp, fp, fp, c_int64, c_int64, c_int64, c_uint64]
        lib.dm_gated_mlp_tail_bwd_widx_f32.restype = c_int32
        lib.dm_gated_mlp_tail_bwd_widx_f32.argtypes = [
            fp, ip, fp, fp, fp, ip, fp, fp, fp, fp, fp, ip, ip, fp,
            POINTER(ctypes.c_double), c_int64, c_int64, c_int64, c_uint64]
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
        # SO(2) convolution on bf16 MFMA (csrc/so2.hip)
        hp = POINTER(ctypes.c_uint16)
        lib.dm_so2_conv_fwd_bf16.restype = c_int32
        lib.dm_so2_conv_fwd_bf16.argtypes = [fp, fp, fp, hp, fp, c_int64,
                                             c_int32, c_uint64]
        lib.dm_so2_conv_bwd_bf16.restype = c_int32
        lib.dm_so2_conv_bwd_bf16.argtypes = [fp, fp, fp, fp, hp, fp, fp, fp,
                                             c_int64, c_int32, c_uint64]
        # S2 grid activation on fp32 MFMA (csrc/s2act.hip)
        lib.dm_s2_act_fwd_f32.restype = c_int32
        lib.dm_s2_act_fwd_f32.argtypes = [fp, fp, fp, fp, c_int64, c_int32,
                                          c_int32, c_uint64]
        lib.dm_s2_act_bwd_f32.restype = c_int32
        lib.dm_s2_act_bwd_f32.argtypes = [fp, fp, fp, fp, fp, c_int64,
                                          c_int32, c_int32, c_uint64]
        lib.dm_mace_symc_fwd_f32.restype = c_int32
        lib.dm_mace_symc_fwd_f32.argtypes = [fp, ip, fp, ip, fp, c_int32,
                                             fp, c_int64, c_int32, c_int32,
                                             c_int32, c_uint64]
        lib.dm_mace_symc_bwd_f32.restype = c_int32
        lib.dm_mace_symc_bwd_f32.argtypes = [fp, fp, ip, fp, ip, fp,
                                             c_int32, fp, c_int64, c_int32,
                                             c_int32, c_int32, c_uint64]
        # tree-factored symmetric contraction (csrc/mace_symc.hip)
        lib.dm_mace_symc_tree_fwd_f32.restype = c_int32
        lib.dm_mace_symc_tree_fwd_f32.argtypes = [fp, ip, fp, ip, fp, c_int64,
                                                  c_int32, c_int32, c_int32,
                                                  c_uint64]
        lib.dm_mace_symc_tree_bwd_f32.restype = c_int32
        lib.dm_mace_symc_tree_bwd_f32.argtypes = [fp, fp, ip, fp, ip, fp,
                                                  c_int64, c_int32, c_int32,
                                                  c_int32, c_uint64]
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
        # MACE fused convolution (distmlip_amd/mace_ops.py, csrc/mace_conv.hip)
        lib.dm_mace_conv_fwd_f32.restype = c_int32
        lib.dm_mace_conv_fwd_f32.argtypes = [fp, fp, fp, fp, ip, ip, fp,
                                             c_int64, c_int32, c_int32,
                                             c_uint64]
        lib.dm_mace_conv_bwd_edge_f32.restype = c_int32
        lib.dm_mace_conv_bwd_edge_f32.argtypes = [fp, fp, fp, fp, fp, ip, ip,
                                                  fp, fp, c_int64, c_int64,
                                                  c_int32, c_int32, c_uint64]
        lib.dm_mace_conv_bwd_node_f32.restype = c_int32
        lib.dm_mace_conv_bwd_node_f32.argtypes = [fp, fp, fp, fp, ip, ip, ip,
                                                  fp, c_int64, c_int32,
                                                  c_int32, c_uint64]
        # the same with the last radial layer inside (h, packed Wr, H)
        lib.dm_mace_conv_rad_fwd_f32.restype = c_int32
        lib.dm_mace_conv_rad_fwd_f32.argtypes = [
            fp, fp, fp, fp, fp, ip, ip, fp, c_int64, c_int32, c_int32,
            c_int32, c_uint64]
        lib.dm_mace_conv_rad_bwd_edge_f32.restype = c_int32
        lib.dm_mace_conv_rad_bwd_edge_f32.argtypes = [
            fp, fp, fp, fp, fp, fp, fp, ip, ip, fp, fp, c_int64, c_int64,
            c_int32, c_int32, c_int32, c_uint64]
        lib.dm_mace_conv_rad_bwd_node_f32.restype = c_int32
        lib.dm_mace_conv_rad_bwd_node_f32.argtypes = [
            fp, fp, fp, fp, fp, ip, ip, ip, fp, c_int64, c_int32, c_int32,
            c_int32, c_uint64]
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
    return ctypes.cast(t.data_ptr(), POINTER(c_float)) if t is not None \
        else None


def _ip(t):
    return ctypes.cast(t.data_ptr(), POINTER(c_int32)) if t is not None \
        else None


def _halves(t):
    """The pointers to t[0] and t[1] of a packed contiguous fp32 [2, ...]
    tensor (cg, w2, b2); (None, None) for None."""
    if t is None:
        return None, None
    p = t.data_ptr()
    return (ctypes.cast(p, POINTER(c_float)),
            ctypes.cast(p + 2 * t.numel(), POINTER(c_float)))


def _hp(t):
    """16-bit words (a bf16 tensor's storage)."""
    return ctypes.cast(t.data_ptr(), POINTER(ctypes.c_uint16))


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
        _fp(msg), _ip(row_ptr), _fp(base), _fp(out), n_rows, msg.shape[1], _stream()), "dm_seg_sum_f32")
    return out


def raw_seg_sum_gather(msg, perm, row_ptr, n_rows, base=None):
    _chk_f32(msg, base)
    out = torch.empty((n_rows,) + tuple(msg.shape[1:]), dtype=msg.dtype,
                      device=msg.device)
    _check(hip_lib().dm_seg_sum_gather_f32(
        _fp(msg), _ip(perm), _ip(row_ptr), _fp(base), _fp(out), n_rows,
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
        _fp(go_h), _fp(go_z), _fp(z), _fp(dz), z.numel(), _stream()),
        "dm_silu_bwd_f32")
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


def _dz_of(go_z, go_h, z):
    """The gradient on z of a first layer that returned (z, silu(z))."""
    if go_h is None:
        return go_z.contiguous()
    return raw_silu_bwd(go_h.contiguous(), _cont(go_z), z)


def _edge_seg_sums(dz, src_perm, src_row_ptr, row_ptr, n_nodes):
    """dz summed onto the src and the dst table of the atom graph."""
    return (raw_seg_sum_gather(dz, src_perm, src_row_ptr, n_nodes),
            raw_seg_sum(dz, row_ptr, n_nodes))


def _line_seg_sums(dz, pd, n_bonds, n_nodes):
    """dz summed onto the l_src, l_dst and center tables of the line graph."""
    return (raw_seg_sum_gather(dz, pd.line_src_perm, pd.line_src_row_ptr,
                               n_bonds),
            raw_seg_sum(dz, pd.line_row_ptr, n_bonds),
            raw_seg_sum_gather(dz, pd.center_perm, pd.center_row_ptr,
                               n_nodes))


def _grad_inputs(*ts):
    return any(t.requires_grad for t in ts)


def raw_gather_add3(zs, zd, ze, src, dst, inplace=False):
    """(z, silu(z)) with z = zs[src] + zd[dst] + ze in one kernel.  inplace:
    silu goes over z (the kernel writes z then silu(z) per element, so one
    buffer is safe and halves the transient footprint) and z is h."""
    _chk_f32(zs, zd, ze)
    z = torch.empty_like(ze)
    h = z if inplace else torch.empty_like(ze)
    _check(hip_lib().dm_gather_add3_f32(
        _fp(zs), _fp(zd), _fp(ze), _ip(src), _ip(dst), _fp(z), _fp(h),
        ze.shape[0], ze.shape[1], _stream()), "dm_gather_add3_f32")
    return z, h


def raw_gather_add4(z1, z2, za, zv, pd, inplace=False):
    """raw_gather_add3 over the line graph's three gathers."""
    _chk_f32(z1, z2, za, zv)
    z = torch.empty_like(za)
    h = z if inplace else torch.empty_like(za)
    _check(hip_lib().dm_gather_add4_f32(
        _fp(z1), _fp(z2), _fp(za), _fp(zv), _ip(pd.l_src), _ip(pd.l_dst),
        _ip(pd.center), _fp(z), _fp(h), za.shape[0], za.shape[1],
        _stream()), "dm_gather_add4_f32")
    return z, h


def raw_edge_mlp3(erow, wt, bias, zs, zd, src, dst, keep_z=True):
    """(z, silu(z)) with z = erow @ wt + bias + zs[src] + zd[dst], the
    per-edge GEMM inside the gather kernel (wt = the [64,128] fusedT pack).
    keep_z=False skips the z write; z is then empty."""
    _chk_f32(erow, wt, bias, zs, zd)
    E, dout = erow.shape[0], wt.shape[1]
    h = torch.empty(E, dout, dtype=erow.dtype, device=erow.device)
    z = torch.empty_like(h) if keep_z else h[:0]
    _check(hip_lib().dm_edge_mlp3_f32(
        _fp(erow), _fp(wt), _fp(bias), _fp(zs), _fp(zd), _ip(src), _ip(dst),
        _fp(z) if keep_z else None, _fp(h), E, wt.shape[0], dout, _stream()),
        "dm_edge_mlp3_f32")
    return z, h


def raw_edge_mlp4(arow, wt, bias, z1, z2, zv, pd):
    """(z, silu(z)) with z = arow @ wt + bias + z1[l_src] + z2[l_dst] +
    zv[center]: raw_edge_mlp3 over the line graph's three gathers."""
    _chk_f32(arow, wt, bias, z1, z2, zv)
    L, dout = arow.shape[0], wt.shape[1]
    h = torch.empty(L, dout, dtype=arow.dtype, device=arow.device)
    z = torch.empty_like(h)
    _check(hip_lib().dm_edge_mlp4_f32(
        _fp(arow), _fp(wt), _fp(bias), _fp(z1), _fp(z2), _fp(zv),
        _ip(pd.l_src), _ip(pd.l_dst), _ip(pd.center), _fp(z), _fp(h), L,
        wt.shape[0], dout, _stream()), "dm_edge_mlp4_f32")
    return z, h


class _GatherAdd3(torch.autograd.Function):
    """Emits (z, silu(z)) in one kernel; z doubles as the saved activation
    for the fused silu backward."""

    @staticmethod
    def forward(ctx, zs, zd, ze, src, dst, src_perm, src_row_ptr, row_ptr):
        # the z output is usually discarded (only h flows on): without this,
        # autograd materializes a full [E,2d] ZERO go_z every backward (a
        # zero-fill write + an extra read inside silu_bwd, ~0.8 ms/call at
        # li100k, rocprof run 17)
        ctx.set_materialize_grads(False)
        ctx.n_nodes = zs.shape[0]
        # grad mode is always OFF inside Function.forward, so test the
        # inputs: when none requires grad (checkpoint outer pass /
        # inference) no backward will run and silu can go in place over z
        z, h = raw_gather_add3(zs, zd, ze, src, dst,
                               inplace=not _grad_inputs(zs, zd, ze))
        ctx.save_for_backward(src_perm, src_row_ptr, row_ptr, z)
        return z, h

    @staticmethod
    def backward(ctx, go_z, go_h):
        src_perm, src_row_ptr, row_ptr, z = ctx.saved_tensors
        dz = _dz_of(go_z, go_h, z)
        gzs, gzd = _edge_seg_sums(dz, src_perm, src_row_ptr, row_ptr,
                                  ctx.n_nodes)
        return gzs, gzd, dz, None, None, None, None, None


def raw_edge_mlp_bwd(dz, wt, gbase=None, out=None, patch=None):
    """out = (gbase +) dz @ wt.t() in ONE kernel: the reverse of the fused
    first layer's per-edge GEMM, with the other gradient of the same rows
    added in its epilogue.  dz [E,128], wt [64,128] (the fusedT pack),
    gbase [E,64] or None.  out may be gbase (in place); only do that with a
    buffer the caller owns.

    patch = (slot, rows): row r of gbase is read from rows[slot[r]] where
    slot[r] >= 0 (slot int32 [E], -1 elsewhere; rows [M,64]; the entries are
    not range-checked: that would cost a device round trip).  rows must not
    share memory with out."""
    _chk_f32(dz, wt, gbase, out)
    E = dz.shape[0]
    assert dz.shape[1] == wt.shape[1]
    assert gbase is None or gbase.shape == (E, wt.shape[0])
    if out is None:
        out = torch.empty(E, wt.shape[0], dtype=dz.dtype, device=dz.device)
    assert out.shape == (E, wt.shape[0])
    if patch is not None:
        slot, rows = patch
        _chk_f32(rows)
        assert gbase is not None, "a patch replaces rows of gbase"
        assert slot.dtype == torch.int32 and slot.is_contiguous() \
            and slot.device == dz.device and slot.shape == (E,)
        assert rows.dim() == 2 and rows.shape[1] == wt.shape[0]
        assert (rows.untyped_storage().data_ptr()
                != out.untyped_storage().data_ptr()), \
            "patch rows must not alias out"
        _check(hip_lib().dm_edge_mlp_bwd_patch_f32(
            _fp(dz), _fp(wt), _fp(gbase), _ip(slot), _fp(rows), _fp(out), E,
            dz.shape[1], wt.shape[0], _stream()), "dm_edge_mlp_bwd_patch_f32")
        return out
    _check(hip_lib().dm_edge_mlp_bwd_f32(
        _fp(dz), _fp(wt), _fp(gbase), _fp(out), E, dz.shape[1], wt.shape[0],
        _stream()), "dm_edge_mlp_bwd_f32")
    return out


def raw_edge_mlp_bwd_src(dz, wt, perm, seg, row_ptr, gbase=None, out=None,
                         patch=None):
    """(raw_edge_mlp_bwd(dz, wt, gbase, out, patch),
    raw_seg_sum_gather(dz, perm, row_ptr, N)) from ONE read of dz: the kernel
    walks the rows in the sorted order perm and sums each node's rows while
    their tile is on chip.  seg int32 [E] is the node of each sorted position
    (the sorted index itself, index[perm]); row_ptr int32 [N+1].  out has the
    bits of raw_edge_mlp_bwd; the sums have those of raw_seg_sum_gather for a
    node whose positions lie within one 32-row tile and are at most 1 ulp off
    for a node spread over several (fp64 pieces added in tile order)."""
    _chk_f32(dz, wt, gbase, out)
    E = dz.shape[0]
    N = row_ptr.shape[0] - 1
    assert dz.shape[1] == wt.shape[1]
    assert gbase is None or gbase.shape == (E, wt.shape[0])
    for t in (perm, seg):
        assert t.dtype == torch.int32 and t.is_contiguous() \
            and t.device == dz.device and t.shape == (E,)
    assert row_ptr.dtype == torch.int32 and row_ptr.is_contiguous() \
        and row_ptr.device == dz.device
    if out is None:
        out = torch.empty(E, wt.shape[0], dtype=dz.dtype, device=dz.device)
    assert out.shape == (E, wt.shape[0])
    slot = rows = None
    if patch is not None:
        slot, rows = patch
        _chk_f32(rows)
        assert gbase is not None, "a patch replaces rows of gbase"
        assert slot.dtype == torch.int32 and slot.is_contiguous() \
            and slot.device == dz.device and slot.shape == (E,)
        assert rows.dim() == 2 and rows.shape[1] == wt.shape[0]
        assert (rows.untyped_storage().data_ptr()
                != out.untyped_storage().data_ptr()), \
            "patch rows must not alias out"
    sums = torch.empty(N, dz.shape[1], dtype=dz.dtype, device=dz.device)
    part = torch.empty(max((E + 31) // 32, 1), 2, dz.shape[1],
                       dtype=torch.float64, device=dz.device)
    _check(hip_lib().dm_edge_mlp_bwd_src_f32(
        _fp(dz), _fp(wt), _fp(gbase), _ip(slot), _fp(rows), _fp(out),
        _ip(perm), _ip(seg), _ip(row_ptr), _fp(sums),
        ctypes.cast(part.data_ptr(), POINTER(ctypes.c_double)), E, N,
        dz.shape[1], wt.shape[0], _stream()), "dm_edge_mlp_bwd_src_f32")
    return out, sums


def _sorted_index(pd, name, index, perm):
    """index[perm] as int32, the node of each sorted position, kept on the
    graph: it changes only when perm does."""
    hit = getattr(pd, name, None)
    if hit is None or hit[0] is not perm:
        hit = (perm, index[perm.long()].to(torch.int32).contiguous())
        setattr(pd, name, hit)
    return hit[1]


def _first_layer_de(dz, wt):
    """dz @ wt.t(): dm_edge_mlp_bwd_f32 for the [64,128] pack where
    mlp_path allows it, else rocBLAS."""
    if (tuple(wt.shape) == (64, 128) and dz.dtype == torch.float32
            and mlp_path.fused_first_bwd(HipOps, wt.shape[0])):
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
        assert not wt.requires_grad and not bias.requires_grad
        ctx.set_materialize_grads(False)
        ctx.n_nodes = zs.shape[0]
        # no backward: skip the z write
        z, h = raw_edge_mlp3(erow, wt, bias, zs, zd, src, dst,
                             keep_z=_grad_inputs(erow, zs, zd))
        ctx.save_for_backward(src_perm, src_row_ptr, row_ptr, z, wt)
        return z, h

    @staticmethod
    def backward(ctx, go_z, go_h):
        src_perm, src_row_ptr, row_ptr, z, wt = ctx.saved_tensors
        dz = _dz_of(go_z, go_h, z)
        de = _first_layer_de(dz, wt)
        gzs, gzd = _edge_seg_sums(dz, src_perm, src_row_ptr, row_ptr,
                                  ctx.n_nodes)
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
        needs_z = _grad_inputs(arow, z1, z2, zv)
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
        z, wt = ctx.saved_tensors
        dz = _dz_of(go_z, go_h, z)
        da = _first_layer_de(dz, wt)
        gz1, gz2, gzv = _line_seg_sums(dz, ctx.pd, ctx.n_bonds, ctx.n_nodes)
        return da, None, None, gz1, gz2, gzv, None


class _GatherAdd4(torch.autograd.Function):
    """Emits (z, silu(z)) over the line-graph 3-gather-add."""

    @staticmethod
    def forward(ctx, z1, z2, za, zv, pd):
        ctx.set_materialize_grads(False)   # see _GatherAdd3.forward
        ctx.pd = pd
        ctx.n_bonds = z1.shape[0]
        ctx.n_nodes = zv.shape[0]
        # see _GatherAdd3.forward: in-place silu only when no backward runs
        z, h = raw_gather_add4(z1, z2, za, zv, pd,
                               inplace=not _grad_inputs(z1, z2, za, zv))
        ctx.save_for_backward(z)
        return z, h

    @staticmethod
    def backward(ctx, go_z, go_h):
        (z,) = ctx.saved_tensors
        dz = _dz_of(go_z, go_h, z)
        gz1, gz2, gzv = _line_seg_sums(dz, ctx.pd, ctx.n_bonds, ctx.n_nodes)
        return gz1, gz2, dz, gzv, None


class _SegSum(torch.autograd.Function):
    """out[n] = base[n] + sum of idx-sorted msg rows in [rp[n], rp[n+1])."""

    @staticmethod
    def forward(ctx, msg, idx, row_ptr, n_rows, base):
        ctx.save_for_backward(idx)
        ctx.has_base = base is not None
        return raw_seg_sum(msg.contiguous(), row_ptr, n_rows,
                           _cont(base))

    @staticmethod
    def backward(ctx, grad):
        (idx,) = ctx.saved_tensors
        gmsg = raw_gather(grad.contiguous(), idx)
        gbase = grad if ctx.has_base else None
        return gmsg, None, None, None, gbase


def _combine_fwd(c_ptr, g_ptr, w, base, out):
    """out = base + silu(c) * sigmoid(g) * w over out.numel() elements."""
    _check(hip_lib().dm_gated_combine_fwd_f32(
        c_ptr, g_ptr, _fp(w), _fp(base), _fp(out), out.numel(), _stream()),
        "dm_gated_combine_fwd_f32")
    return out


def _combine_bwd(go, c_ptr, g_ptr, w, dc_ptr, dg_ptr):
    """Writes dc and dg through their pointers; returns dw (None without w)."""
    dw = torch.empty_like(w) if w is not None else None
    _check(hip_lib().dm_gated_combine_bwd_f32(
        _fp(go), c_ptr, g_ptr, _fp(w), dc_ptr, dg_ptr, _fp(dw), go.numel(),
        _stream()), "dm_gated_combine_bwd_f32")
    return dw


def raw_combine_fwd(cg, w, base):
    """base + silu(cg[0]) * sigmoid(cg[1]) * w over packed cg [2,E,D]."""
    _chk_f32(cg, w, base)
    return _combine_fwd(*_halves(cg), w, base, torch.empty(
        cg.shape[1], cg.shape[2], dtype=cg.dtype, device=cg.device))


def raw_combine_bwd(go, cg, w):
    """(dcg [2,E,D] packed, dw) from the gradient go of raw_combine_fwd."""
    _chk_f32(go, cg, w)
    dcg = torch.empty_like(cg)
    return dcg, _combine_bwd(go, *_halves(cg), w, *_halves(dcg))


class _GatedCombine(torch.autograd.Function):
    """out = base + silu(c) * sigmoid(g) * w — fused gated-MLP epilogue."""

    @staticmethod
    def forward(ctx, c, g, w, base):
        _chk_f32(c, g, w, base)
        ctx.save_for_backward(c, g, w)
        ctx.has_base = base is not None
        return _combine_fwd(_fp(c), _fp(g), w, base, torch.empty_like(c))

    @staticmethod
    def backward(ctx, go):
        c, g, w = ctx.saved_tensors
        go = go.contiguous()
        dc = torch.empty_like(c)
        dg = torch.empty_like(g)
        dw = _combine_bwd(go, _fp(c), _fp(g), w, _fp(dc), _fp(dg))
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
        ctx.save_for_backward(cg, w)
        ctx.has_base = base is not None
        return raw_combine_fwd(cg, w, base)

    @staticmethod
    def backward(ctx, go):
        cg, w = ctx.saved_tensors
        go = go.contiguous()
        dcg, dw = raw_combine_bwd(go, cg, w)
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
    added onto dbexp_acc in place when that is given.  With seg (a graph
    whose dst-sorted rows are the tail's: with_seg) r_mlp_tail_bwd returns
    (dz, dbexp, r_seg_dst(dz, seg)), the sums from the kernel's epilogue."""

    __slots__ = ("bexp", "W", "mask", "dbexp_acc", "seg")

    def __init__(self, bexp, W, mask=None, dbexp_acc=None, seg=None):
        self.bexp, self.W, self.dbexp_acc = bexp, W, dbexp_acc
        self.mask = mask.reshape(-1) if mask is not None else None
        self.seg = seg

    @property
    def requires_grad(self):
        return self.bexp.requires_grad

    def with_acc(self, dbexp_acc):
        return RadialW(self.bexp, self.W, self.mask, dbexp_acc, self.seg)

    def with_seg(self, pd):
        return RadialW(self.bexp, self.W, self.mask, self.dbexp_acc, pd)

    def check(self, E, d):
        _chk_f32(self.bexp, self.W, self.mask, self.dbexp_acc)
        assert self.bexp.shape[0] == E and self.W.shape == (
            d, self.bexp.shape[1])
        assert self.mask is None or self.mask.shape == (E,)
        assert self.dbexp_acc is None \
            or self.dbexp_acc.shape == self.bexp.shape

    def ptrs(self):
        return _fp(self.bexp), _fp(self.W), _fp(self.mask)


def _split_w(w):
    """(dense w or None, RadialW or None) of a tail's w argument."""
    return (None, w) if isinstance(w, RadialW) else (w, None)


def _chk_w_idx(w, w_idx, E, d):
    """w [T,d] dense with w_idx int32 [E]: row r of the kernel takes
    w[w_idx[r]].  The range of w_idx is the caller's to guarantee (graph
    indices), as for every gather index."""
    assert w is not None and not isinstance(w, RadialW) \
        and w.dim() == 2 and w.shape[1] == d and w.shape[0] > 0
    assert w_idx.dtype == torch.int32 and w_idx.is_contiguous() \
        and w_idx.device == w.device and w_idx.shape == (E,)


class LineSeg:
    """The line graph's dst-sorted rows as the seg of raw_mlp_tail_bwd."""

    def __init__(self, pd):
        self.dst, self.row_ptr, self.n_atoms = (pd.l_dst, pd.line_row_ptr,
                                                pd.n_bonds)


def raw_mlp_tail_bwd(go, cg, w, z, w2, go_idx=None, seg=None, w_idx=None):
    """(dz, dw) of one gated MLP's tail in ONE kernel: the reverse of
    out = base + silu(cg[0]) * sigmoid(cg[1]) * w with cg = the second layer
    over silu(z).  go [E,d], cg [2,E,d] packed, w [E,d] or None, z [E,2d],
    w2 [2,d,d] (input x output per half).  d must be 64.  With go_idx
    (int32 [E]) go is a [N,d] table and row r takes go[go_idx[r]]: the
    result on the materialized go[go_idx], without that gather.
    w may be a RadialW: (dz, dbexp) is returned then.
    seg (a graph with dst int32 [E] sorted, row_ptr int32 [N+1] and n_atoms;
    a RadialW brings its own) adds raw_seg_sum(dz, seg.row_ptr, N) as a third
    result, summed in the kernel's epilogue from the registers that hold dz
    and finished by a pass over per-tile fp64 partials: the bits of
    raw_seg_sum for a node whose rows lie within one 32-row tile, at most
    1 ulp off for a node spread over several.  It needs a w.
    w_idx (int32 [E]): the dense w is a [T,d] table and row r takes
    w[w_idx[r]]; dz and dw ([E,d], one row per r) are those of the
    materialized w[w_idx]."""
    w, rw = _split_w(w)
    if rw is not None and seg is None:
        seg = rw.seg
    _chk_f32(go, cg, w, z, w2)
    d = go.shape[1]
    E = go.shape[0] if go_idx is None else go_idx.shape[0]
    assert cg.shape == (2, E, d) and z.shape == (E, 2 * d)
    assert w2.shape == (2, d, d)
    assert w_idx is not None or w is None or w.shape == (E, d)
    if go_idx is not None:
        assert go_idx.dtype == torch.int32 and go_idx.is_contiguous() \
            and go_idx.device == go.device
    dz = torch.empty_like(z)
    lib = hip_lib()
    if seg is not None:
        assert seg.dst.shape == (E,) and seg.dst.dtype == torch.int32 \
            and seg.row_ptr.dtype == torch.int32 \
            and seg.row_ptr.shape == (seg.n_atoms + 1,)
    if w_idx is not None:
        _chk_w_idx(w, w_idx, E, d)
        dw = torch.empty(E, d, dtype=z.dtype, device=z.device)
        sums = part = None
        if seg is not None:
            sums = torch.empty(seg.n_atoms, 2 * d, dtype=z.dtype,
                               device=z.device)
            part = torch.empty((E + 31) // 32, 2, 2 * d, dtype=torch.float64,
                               device=z.device)
        _check(lib.dm_gated_mlp_tail_bwd_widx_f32(
            _fp(go), _ip(go_idx), *_halves(cg), _fp(w), _ip(w_idx), _fp(z),
            *_halves(w2), _fp(dz), _fp(dw),
            _ip(seg.dst) if seg is not None else None,
            _ip(seg.row_ptr) if seg is not None else None, _fp(sums),
            ctypes.cast(part.data_ptr(), POINTER(ctypes.c_double))
            if part is not None else None, E,
            seg.n_atoms if seg is not None else 0, d, _stream()),
            "dm_gated_mlp_tail_bwd_widx_f32")
        return (dz, dw, sums) if seg is not None else (dz, dw)
    if seg is not None:
        acc = dw = dbexp = None
        if rw is not None:
            rw.check(E, d)
            acc = rw.dbexp_acc
            dbexp = acc if acc is not None else torch.empty_like(rw.bexp)
        else:
            dw = torch.empty_like(w)
        sums = torch.empty(seg.n_atoms, 2 * d, dtype=z.dtype, device=z.device)
        part = torch.empty((E + 31) // 32, 2, 2 * d, dtype=torch.float64,
                           device=z.device)
        _check(lib.dm_gated_mlp_tail_bwd_seg_f32(
            _fp(go), _ip(go_idx), *_halves(cg), _fp(w),
            *(rw.ptrs() if rw is not None else (None, None, None)), _fp(z),
            *_halves(w2), _fp(dz), _fp(dw), _fp(acc), _fp(dbexp),
            _ip(seg.dst), _ip(seg.row_ptr), _fp(sums),
            ctypes.cast(part.data_ptr(), POINTER(ctypes.c_double)), E,
            seg.n_atoms, d, rw.bexp.shape[1] if rw is not None else 0,
            _stream()), "dm_gated_mlp_tail_bwd_seg_f32")
        return dz, (dbexp if rw is not None else dw), sums
    if rw is not None:
        rw.check(E, d)
        acc = rw.dbexp_acc
        dbexp = acc if acc is not None else torch.empty_like(rw.bexp)
        _check(lib.dm_gated_mlp_tail_bwd_fw_f32(
            _fp(go), _ip(go_idx), *_halves(cg), *rw.ptrs(), _fp(z),
            *_halves(w2), _fp(dz), _fp(acc), _fp(dbexp), E, d,
            rw.bexp.shape[1], _stream()), "dm_gated_mlp_tail_bwd_fw_f32")
        return dz, dbexp
    dw = torch.empty_like(w) if w is not None else None
    rest = (*_halves(cg), _fp(w), _fp(z), *_halves(w2), _fp(dz), _fp(dw), E,
            d, _stream())
    if go_idx is not None:
        _check(lib.dm_gated_mlp_tail_bwd_idx_f32(_fp(go), _ip(go_idx), *rest),
               "dm_gated_mlp_tail_bwd_idx_f32")
    else:
        _check(lib.dm_gated_mlp_tail_bwd_f32(_fp(go), *rest),
               "dm_gated_mlp_tail_bwd_f32")
    return dz, dw


def raw_mlp_tail_fwd(h, w2, b2, w, base, keep_cg, w_idx=None):
    """(out, cg or None) of one gated MLP's tail in ONE kernel:
    cg = baddbmm(b2, h halves, w2) and out = base + silu(cg[0]) *
    sigmoid(cg[1]) * w.  h [E,2d], w2 [2,d,d] (input x output per half),
    b2 [2,1,d], w and base [E,d] or None.  cg [2,E,d] packed is written and
    returned only with keep_cg; out is the same bit for bit either way.
    d must be 64.  w may be a RadialW, or with w_idx (int32 [E]) a [T,d] table
    of which row r takes w[w_idx[r]]."""
    w, rw = _split_w(w)
    _chk_f32(h, w2, b2, w, base)
    E, d = h.shape[0], w2.shape[1]
    assert h.shape == (E, 2 * d) and w2.shape == (2, d, d)
    assert b2.numel() == 2 * d
    assert w_idx is not None or w is None or w.shape == (E, d)
    assert base is None or base.shape == (E, d)
    out = torch.empty(E, d, dtype=h.dtype, device=h.device)
    cg = torch.empty(2, E, d, dtype=h.dtype, device=h.device) \
        if keep_cg else None
    head = (_fp(h), *_halves(w2), *_halves(b2))
    rest = (_fp(base), *_halves(cg), _fp(out), E, d)
    if w_idx is not None:
        _chk_w_idx(w, w_idx, E, d)
        _check(hip_lib().dm_gated_mlp_tail_fwd_widx_f32(
            *head, _fp(w), _ip(w_idx), *rest, _stream()),
            "dm_gated_mlp_tail_fwd_widx_f32")
    elif rw is not None:
        rw.check(E, d)
        _check(hip_lib().dm_gated_mlp_tail_fwd_fw_f32(
            *head, *rw.ptrs(), *rest, rw.bexp.shape[1], _stream()),
            "dm_gated_mlp_tail_fwd_fw_f32")
    else:
        _check(hip_lib().dm_gated_mlp_tail_fwd_f32(
            *head, _fp(w), *rest, _stream()), "dm_gated_mlp_tail_fwd_f32")
    return out, cg


def raw_gated_mlp(row, wt, bias, tables, idx, w2, b2, w, base, keep,
                  want_out=True, w_idx=None):
    """One whole gated MLP in ONE kernel (dm_gated_mlp3/4_f32): the fused
    first layer over row [E,64] and 2 or 3 gathered tables, the second layer
    and the combine, without the h [E,128] array between them.  Returns
    (z, cg, out): z [E,128] and cg [2,E,64] packed with keep, else None; out
    None with want_out=False (keep only; w and base are then not read).
    Values are the two-kernel path's bit for bit.  w may be a RadialW (two
    tables, with out), or with w_idx (int32 [E]; three tables, with out, no
    base) a [T,d] table of which row r takes w[w_idx[r]]."""
    w, rw = _split_w(w)
    if not want_out:
        w = rw = base = w_idx = None
    _chk_f32(row, wt, bias, *tables, w2, b2, w, base)
    E, d = row.shape[0], w2.shape[1]
    assert wt.shape == (d, 2 * d) and w2.shape == (2, d, d)
    assert b2.numel() == 2 * d and bias.numel() == 2 * d
    assert len(tables) == len(idx) and len(tables) in (2, 3)
    assert all(t.shape[1] == 2 * d for t in tables)
    assert keep or want_out
    assert w_idx is not None or w is None or w.shape == (E, d)
    if w_idx is not None:
        assert len(tables) == 3 and base is None, \
            "w_idx takes the three-gather form without base"
        _chk_w_idx(w, w_idx, E, d)
    assert base is None or base.shape == (E, d)
    z = torch.empty(E, 2 * d, dtype=row.dtype, device=row.device) \
        if keep else None
    if E == 0:
        e0 = row.new_empty
        return z, e0(2, 0, d) if keep else None, e0(0, d) if want_out else None
    cg = torch.empty(2, E, d, dtype=row.dtype, device=row.device) \
        if keep else None
    out = torch.empty(E, d, dtype=row.dtype, device=row.device) \
        if want_out else None
    first = (_fp(row), _fp(wt), _fp(bias), *map(_fp, tables),
             *map(_ip, idx), *_halves(w2), *_halves(b2))
    rest = (_fp(base), _fp(z), *_halves(cg), _fp(out), E, wt.shape[0], d)
    if w_idx is not None:
        _check(hip_lib().dm_gated_mlp4_widx_f32(
            *first, _fp(w), _ip(w_idx), *rest, _stream()),
            "dm_gated_mlp4_widx_f32")
    elif rw is not None:
        assert len(tables) == 2, "a factored w takes the two-gather form"
        rw.check(E, d)
        _check(hip_lib().dm_gated_mlp3_fw_f32(
            *first, *rw.ptrs(), *rest, rw.bexp.shape[1], _stream()),
            "dm_gated_mlp3_fw_f32")
    elif len(tables) == 2:
        _check(hip_lib().dm_gated_mlp3_f32(*first, _fp(w), *rest, _stream()),
               "dm_gated_mlp3_f32")
    else:
        _check(hip_lib().dm_gated_mlp4_f32(*first, _fp(w), *rest, _stream()),
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
    writes cg for the backward and never reads it back (where
    mlp_path.fused_tail_fwd says no: baddbmm + raw_combine_fwd, as in
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
        if mlp_path.fused_tail_fwd(HipOps, d):
            out, cg = raw_mlp_tail_fwd(h, w2, b2, w, base, True)
        else:
            cg = torch.baddbmm(b2, h.view(-1, 2, d).transpose(0, 1), w2)
            out = raw_combine_fwd(cg, w, base)
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
    tail_bwd_seg = True          # ... and may carry a graph (with_seg);
                                 # a dense w takes seg= (ops.LineSeg)
    w_idx = True                 # a dense w may be a table read by w_idx

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
            z, h, w2, b2, _cont(w), _cont(base))

    def mlp_tail_act(self, h, w2, b2, w=None, base=None, w_idx=None):
        """mlp_tail's value for passes that record nothing (torch.no_grad
        inference, the lean recompute forwards of conv.py): out only, no cg is
        allocated or written.  Not differentiable: refused when an input
        would need a gradient."""
        assert not (torch.is_grad_enabled() and any(
            t is not None and t.requires_grad for t in (h, w, base))), \
            "mlp_tail_act is the no-grad form; use mlp_tail"
        if not isinstance(w, RadialW):
            w = _cont(w)
        kw = {"w_idx": w_idx} if w_idx is not None else {}
        return raw_mlp_tail_fwd(
            h.contiguous(), w2, b2, w,
            _cont(base), False, **kw)[0]

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
        return raw_gather_add3(zs, zd, ze, pd.src, pd.dst)

    def r_combine_fwd(self, cg, w, base):
        return raw_combine_fwd(cg, w, base)

    def r_combine_bwd(self, go, cg, w):
        return raw_combine_bwd(go, cg, w)

    def r_silu_bwd(self, go_h, z):
        return raw_silu_bwd(go_h.contiguous(), None, z)

    def r_mlp_tail_bwd(self, go, cg, w, z, w2, go_idx=None, w_idx=None,
                       seg=None):
        """(dz, dw): r_combine_bwd + second-layer reverse + r_silu_bwd in
        one kernel (d = 64 only).  go_idx: go is a node table read by index
        (r_gather_dst folded in).  With w a RadialW: (dz, dbexp), and with
        one that carries a graph (with_seg): (dz, dbexp, r_seg_dst(dz)).
        w_idx: the dense w is a table read by index (dw stays per row).
        seg (dense w; LineSeg): the segment sums of dz as a third result."""
        return raw_mlp_tail_bwd(go, cg, w, z, w2, go_idx, seg, w_idx)

    def r_edge_mlp3(self, erow, wt, bias, zs, zd, pd):
        """(z, h) of the fused first layer with z stored: r_gather_add3
        over addmm(bias, erow, wt) without that [E,2d] transient (wt =
        the [64,128] fusedT pack only)."""
        return raw_edge_mlp3(erow, wt, bias, zs, zd, pd.src, pd.dst)

    def r_edge_mlp4(self, arow, wt, bias, z1, z2, zv, pd):
        """r_edge_mlp3 over the line graph's three gathers."""
        return raw_edge_mlp4(arow, wt, bias, z1, z2, zv, pd)

    # r_edge_mlp_bwd takes patch=(slot, rows)
    edge_mlp_bwd_patch = True

    def r_edge_mlp_bwd(self, dz, wt, gbase=None, out=None, patch=None,
                       src=None):
        """(gbase +) dz @ wt.t() in one kernel (wt = the [64,128] fusedT
        pack only); out may be gbase when the caller owns it.  patch =
        (slot, rows): gbase row r is rows[slot[r]] where slot[r] >= 0.
        src = (perm, seg, row_ptr), from r_edge_mlp_bwd_src: the pair
        raw_edge_mlp_bwd_src returns."""
        if src is not None:
            return raw_edge_mlp_bwd_src(dz, wt, *src, gbase, out, patch)
        return raw_edge_mlp_bwd(dz, wt, gbase, out, patch)

    def r_edge_mlp_bwd_src(self, dz, wt, gbase, pd, out=None, patch=None,
                           line=False):
        """(r_edge_mlp_bwd(dz, wt, gbase, out, patch), r_seg_src(dz, pd)) in
        one kernel that reads dz once; line=True: r_seg_lsrc(dz, pd).  It is
        a launch of r_edge_mlp_bwd, and goes through it."""
        if line:
            perm, rp = pd.line_src_perm, pd.line_src_row_ptr
            seg = _sorted_index(pd, "_line_src_seg", pd.l_src, perm)
        else:
            perm, rp = pd.src_perm, pd.src_row_ptr
            seg = _sorted_index(pd, "_src_seg", pd.src, perm)
        return self.r_edge_mlp_bwd(dz, wt, gbase, out, patch=patch,
                                   src=(perm, seg, rp))

    def r_move_rows(self, src, si, dst, di, add=False):
        """dst[di] (=|+=) src[si] by rows, in place over dst, one kernel;
        si / di int64 or None (identity), di unique."""
        return raw_move_rows(src, si, dst, di, add)

    def r_zero_rows(self, dst, di):
        """dst[di] = 0 by rows, in place, one kernel."""
        return raw_zero_rows(dst, di)

    def r_mlp_tail_fwd(self, h, w2, b2, w, base, w_idx=None):
        """(cg, out): second layer + r_combine_fwd in one kernel (d = 64
        only).  w_idx: the dense w is a table read by index."""
        kw = {"w_idx": w_idx} if w_idx is not None else {}
        out, cg = raw_mlp_tail_fwd(h, w2, b2, w, base, True, **kw)
        return cg, out

    # whole gated MLP in one kernel (first layer, second layer, combine)

    def gated_mlp4_act(self, arow, wt, bias, z1, z2, zv, pd, w2, b2, w=None,
                       base=None, w_idx=None):
        """mlp_tail_act(edge_mlp4_act(...), w2, b2, w, base) in one kernel,
        h never reaching memory; for passes that record nothing.  w_idx
        (without base): w is a table read by index."""
        assert _no_grad_inputs(arow, z1, z2, zv, w, base), \
            "gated_mlp4_act is the no-grad form"
        return raw_gated_mlp(arow.contiguous(), wt, bias,
                             (z1.contiguous(), z2.contiguous(),
                              zv.contiguous()),
                             (pd.l_src, pd.l_dst, pd.center), w2, b2,
                             _cont(w), _cont(base), False, w_idx=w_idx)[2]

    def r_gated_mlp4(self, arow, wt, bias, z1, z2, zv, pd, w2, b2, w, base,
                     w_idx=None, want_out=True):
        """(z, cg, out) of the fused three-gather first layer +
        r_mlp_tail_fwd in one kernel, the keep form of gated_mlp4_act: same
        out bit for bit; out is None with want_out=False, and w and base are
        then not read."""
        return raw_gated_mlp(arow, wt, bias, (z1, z2, zv),
                             (pd.l_src, pd.l_dst, pd.center), w2, b2, w, base,
                             True, want_out, w_idx)

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
        return raw_gather_add4(z1, z2, za, zv, pd)

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
            _cont(w), _cont(base))

    def gated_combine_packed(self, cg, w=None, base=None):
        return _GatedCombinePacked.apply(
            cg.contiguous(),
            _cont(w), _cont(base))

    def edge_geom_rbf(self, pos, offshift, freqs, cutoff, pexp, pd):
        return _EdgeGeomRbf.apply(pos.contiguous(), offshift.contiguous(),
                                  freqs.contiguous(), cutoff, pexp, pd)

    def rbf_env(self, d, freqs, cutoff, pexp):
        return _RbfEnv.apply(d.contiguous(), freqs.contiguous(), cutoff, pexp)
