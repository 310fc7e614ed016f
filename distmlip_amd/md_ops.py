"""Integrator ops of the native MD / relaxation driver (distmlip_amd/md.py).

Two functions, each with two implementations chosen by the state's device:

  kick_drift   v = a v + b F/m, drift (plain, or the Langevin "AOA" middle
               of a BAOAB step when noise `xi` is given), cartesian ->
               fractional, periodic wrap into [0,1).  Updates frac and vel
               IN PLACE.
  kick_reduce  v += b F/m (in place; b == 0 is a pure reduction) and returns
               a device fp64 tensor [5]:
               sum m v^2, sum F.v, sum |F|^2, sum |v|^2, max_i |F_i|^2.

On a CPU device both are an fp64 torch composition (`*_torch`).  On a
`cuda` device they are the HIP kernels dm_md_kick_drift_f64 /
dm_md_kick_reduce_f64 (include/distmlip_hip.h); a missing library is an
error there, as everywhere else in the package.  The composition performs
the kernels' operations in the kernels' order, one rounding per operation,
so per atom the two agree to the bit; it is the reference the kernel tests
compare against (it runs on any device).

State is fp64: frac [N,3] wrapped fractional, vel [N,3] cartesian (A/fs),
inv_mass [N] or None (unit masses, FIRE).  `force` [N,3] is fp32 or fp64.
The unit factor (eV/A/amu -> A/fs^2) is the caller's: it is folded into b.

The wrap: on a periodic dim f -= floor(f); that rounds to exactly 1.0 for a
tiny negative f, so a result >= 1.0 becomes 0.0.  The graph builder's
contract is frac in [0,1) on periodic dims (gpu_graph.supported()).
"""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_double, c_int32, c_int64

import numpy as np
import torch

BLOCK = 256          # atoms per block of the HIP kernels
NRED = 5             # m v^2, F.v, |F|^2, |v|^2, max |F_i|^2


def _check_state(frac, vel, force, inv_mass, xi=None):
    N = vel.shape[0]
    for name, t, shape in (("frac", frac, (N, 3)), ("vel", vel, (N, 3)),
                           ("inv_mass", inv_mass, (N,)), ("xi", xi, (N, 3))):
        if t is None:
            continue
        if t.dtype != torch.float64 or tuple(t.shape) != shape \
                or not t.is_contiguous() or t.device != vel.device:
            raise ValueError(f"{name} must be a contiguous fp64 {shape} "
                             f"tensor on {vel.device}")
    if tuple(force.shape) != (N, 3) or force.device != vel.device \
            or force.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"force must be fp32/fp64 {(N, 3)} on {vel.device}, "
                         f"got {force.dtype} {tuple(force.shape)} on "
                         f"{force.device}")


# ---------------------------------------------------------------------------
# fp64 torch composition (CPU path; reference of the kernel tests)
# ---------------------------------------------------------------------------

def kick_drift_torch(frac, vel, force, inv_mass, a, b, h, linv, pbc,
                     xi=None, c1=0.0, c2=0.0):
    _check_state(frac, vel, force, inv_mass, xi)
    F = force.to(torch.float64)
    t = (inv_mass * b).unsqueeze(1) if inv_mass is not None else b
    v = vel * a + F * t
    if xi is not None:
        hh = 0.5 * h
        s = (torch.sqrt(inv_mass) * c2).unsqueeze(1) \
            if inv_mass is not None else c2
        d1 = v * hh
        v = v * c1 + xi * s
        dr = d1 + v * hh
    else:
        dr = v * h
    vel.copy_(v)
    li = np.asarray(linv, dtype=np.float64).reshape(3, 3)
    for k in range(3):
        df = (dr[:, 0] * float(li[0, k]) + dr[:, 1] * float(li[1, k])) \
            + dr[:, 2] * float(li[2, k])
        f = frac[:, k] + df
        if int(pbc[k]):
            f = f - torch.floor(f)
            f = torch.where(f >= 1.0, torch.zeros_like(f), f)
        frac[:, k] = f


def kick_reduce_torch(vel, force, inv_mass, b):
    _check_state(None, vel, force, inv_mass)
    F = force.to(torch.float64)
    if b != 0.0:
        t = (inv_mass * b).unsqueeze(1) if inv_mass is not None else b
        vel.add_(F * t)
    v = vel
    v2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    mv2 = v2 / inv_mass if inv_mass is not None else v2
    fv = (F[:, 0] * v[:, 0] + F[:, 1] * v[:, 1]) + F[:, 2] * v[:, 2]
    f2 = (F[:, 0] * F[:, 0] + F[:, 1] * F[:, 1]) + F[:, 2] * F[:, 2]
    if v.shape[0] == 0:
        return torch.zeros(NRED, dtype=torch.float64, device=v.device)
    return torch.stack([mv2.sum(), fv.sum(), f2.sum(), v2.sum(), f2.max()])


# ---------------------------------------------------------------------------
# HIP kernels
# ---------------------------------------------------------------------------

def _dp(t):
    return ctypes.cast(t.data_ptr(), POINTER(c_double)) if t is not None \
        else None


def _host_cell(linv, pbc):
    li = np.ascontiguousarray(np.asarray(linv, dtype=np.float64).reshape(9))
    pb = np.ascontiguousarray([1 if int(x) else 0 for x in pbc],
                              dtype=np.int32)
    return li, pb


def _hip_force(force):
    if not force.is_contiguous():
        force = force.contiguous()
    return force, ctypes.c_void_p(force.data_ptr()), \
        c_int32(1 if force.dtype == torch.float64 else 0)


def kick_drift_hip(frac, vel, force, inv_mass, a, b, h, linv, pbc,
                   xi=None, c1=0.0, c2=0.0):
    from distmlip_amd.ops import _check, _stream, hip_lib
    _check_state(frac, vel, force, inv_mass, xi)
    if vel.device.type != "cuda":
        raise RuntimeError("kick_drift_hip needs device tensors")
    lib = hip_lib()
    li, pb = _host_cell(linv, pbc)
    force, fptr, f64 = _hip_force(force)
    with torch.cuda.device(vel.device):
        _check(lib.dm_md_kick_drift_f64(
            _dp(frac), _dp(vel), fptr, f64, _dp(inv_mass), _dp(xi),
            c_double(a), c_double(b), c_double(h), c_double(c1), c_double(c2),
            li.ctypes.data_as(POINTER(c_double)),
            pb.ctypes.data_as(POINTER(c_int32)), c_int64(vel.shape[0]),
            _stream()), "dm_md_kick_drift_f64")


def kick_reduce_hip(vel, force, inv_mass, b):
    from distmlip_amd.ops import _check, _stream, hip_lib
    _check_state(None, vel, force, inv_mass)
    if vel.device.type != "cuda":
        raise RuntimeError("kick_reduce_hip needs device tensors")
    lib = hip_lib()
    N = vel.shape[0]
    nb = (N + BLOCK - 1) // BLOCK
    force, fptr, f64 = _hip_force(force)
    with torch.cuda.device(vel.device):
        partials = torch.empty((NRED, max(nb, 1)), dtype=torch.float64,
                               device=vel.device)
        out = torch.empty(NRED, dtype=torch.float64, device=vel.device)
        _check(lib.dm_md_kick_reduce_f64(
            _dp(vel), fptr, f64, _dp(inv_mass), c_double(b), _dp(partials),
            _dp(out), c_int64(N), _stream()), "dm_md_kick_reduce_f64")
    return out


# ---------------------------------------------------------------------------
# dispatch by device
# ---------------------------------------------------------------------------

def kick_drift(frac, vel, force, inv_mass, a, b, h, linv, pbc, xi=None,
               c1=0.0, c2=0.0):
    fn = kick_drift_hip if vel.device.type == "cuda" else kick_drift_torch
    fn(frac, vel, force, inv_mass, a, b, h, linv, pbc, xi=xi, c1=c1, c2=c2)


def kick_reduce(vel, force, inv_mass, b):
    fn = kick_reduce_hip if vel.device.type == "cuda" else kick_reduce_torch
    return fn(vel, force, inv_mass, b)
