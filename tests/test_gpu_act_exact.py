"""GPU tests of the exact sigmoid / SiLU the CHGNet kernels share (sigf / siluf
in csrc/kernels.hip): a shorter instruction sequence that must return the bits
of 1/(1+expf(-x)) and x/(1+expf(-x)) for every fp32 input.

* Exhaustive: dm_act_check_f32 over all 2^32 bit patterns, both functions.
* Through the kernels: the full-tile and the tail epilogues are separate code
  copies, and a wave leaves the short sequence as a whole when one of its
  lanes is out of range.  Values at and beyond every threshold of either form
  are planted in the first row and in the last row (the ragged tile where there
  is one) of otherwise ordinary inputs, and each kernel's output is compared
  bit for bit with the plain expression applied to the kernel's own
  pre-activation, one torch fp32 operation per rounding.  Two NaNs count as
  equal; nothing else is tolerated.
"""
import ctypes
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs HIP GPU")

D = 64
ROWS = [1, 31, 32, 33, 65]
SIG, SILU = 0, 1
FLT_MAX = 3.4028234663852886e38
FLT_MIN = 1.1754943508222875e-38
SUB_MIN = 1.401298464324817e-45          # bits 0x00000001
SUB_MAX = 1.1754942106924411e-38         # bits 0x007fffff
# zero, the subnormal range, the smallest normal, a small normal, the point
# where 1 + exp(-x) stops changing (16.7), the ends of the short sequence's
# range (87.3), expf's overflow threshold from both sides (88.7, 88.73) and its
# underflow threshold from both sides (103.9, 104), the largest finite, inf
MAGNITUDES = [0.0, SUB_MIN, SUB_MAX, FLT_MIN, 1e-30, 16.7, 87.3, 88.7, 88.73,
              103.9, 104.0, FLT_MAX, float("inf")]
FINITE = [m for m in MAGNITUDES if m != float("inf")]


def _signed(mags):
    return torch.tensor([s * m for m in mags for s in (1.0, -1.0)],
                        dtype=torch.float32)


def _pattern(mags, n, shift=0):
    v = _signed(mags)
    return v[(torch.arange(n) + shift) % len(v)]


def _fp(t, off=0):
    if t is None:
        return None
    return ctypes.cast(t.data_ptr() + 4 * off, ctypes.POINTER(ctypes.c_float))


def _ip(t):
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_int32))


def _assert_same_bits(got, want, what):
    same = (got.view(torch.int32) == want.view(torch.int32)) \
        | (got.isnan() & want.isnan())
    if not bool(same.all()):
        i = int((~same).flatten().nonzero()[0])
        g = got.flatten()[i].view(torch.int32).item() & 0xffffffff
        w = want.flatten()[i].view(torch.int32).item() & 0xffffffff
        raise AssertionError(
            f"{what}: {int((~same).sum())} elements differ, first at flat "
            f"index {i}: got 0x{g:08x}, expected 0x{w:08x}")


def _plant(t, mags, shift=0):
    """Special values across the first and (reversed) the last row of t."""
    n = t.shape[1]
    t[0] = _pattern(mags, n, shift).to(t.device)
    t[-1] = _pattern(mags, n, shift).flip(0).to(t.device)
    return t


@requires_gpu
@pytest.mark.parametrize("which", [SIG, SILU])
def test_exhaustive(which):
    """Every one of the 2^32 fp32 bit patterns, in four launches."""
    from distmlip_amd.ops import raw_act_check, raw_act_eval
    bad, first = 0, None
    for chunk in range(4):
        n, lo = raw_act_check(which, chunk << 30, 1 << 30)
        bad += n
        if lo is not None and first is None:
            first = lo
    if bad:
        value, = struct.unpack("f", struct.pack("I", first))
        x = torch.tensor([value], dtype=torch.float32).cuda()
        new = raw_act_eval(which, x, ref=False).view(torch.int32).item()
        ref = raw_act_eval(which, x, ref=True).view(torch.int32).item()
        name = "siluf" if which else "sigf"
        print(f"{name}: {bad} mismatches, first x = 0x{first:08x}: "
              f"kernels' 0x{new & 0xffffffff:08x}, "
              f"plain 0x{ref & 0xffffffff:08x}")
    assert bad == 0


@requires_gpu
def test_eval_entry_specials():
    """dm_act_eval_f32 itself: both forms agree on the planted values, and the
    plain form gives what the expression gives at values with known results."""
    from distmlip_amd.ops import raw_act_eval
    x = _signed(MAGNITUDES).cuda()
    for which in (SIG, SILU):
        _assert_same_bits(raw_act_eval(which, x, ref=False),
                          raw_act_eval(which, x, ref=True), f"which={which}")
    s = raw_act_eval(SIG, torch.tensor([0.0, float("inf"), -float("inf"),
                                        104.0, -104.0]).cuda(), ref=True)
    assert s.tolist() == [0.5, 1.0, 0.0, 1.0, 0.0]
    assert bool(raw_act_eval(SILU, torch.tensor([float("nan")]).cuda(),
                             ref=False).isnan().all())
    assert bool(raw_act_eval(SIG, torch.tensor([float("nan")]).cuda(),
                             ref=False).isnan().all())


@requires_gpu
@pytest.mark.parametrize("E", ROWS)
def test_edge_mlp_h_is_silu_of_its_z(E):
    """h of dm_edge_mlp3_f32 against the plain SiLU of its own z.  The
    special values reach z through the gathered table (a product with an
    identity WT would turn the row with inf into NaN): the planted rows have a
    zero e-row and gather table row 1, the rest gather the zero row 0."""
    from distmlip_amd.ops import _stream, hip_lib, raw_act_eval
    lib = hip_lib()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(501 + E)
    erow = (3 * torch.randn(E, D, generator=gen)).to(dev)
    erow[0] = 0
    erow[-1] = 0
    eye = torch.eye(D)
    wt = torch.cat([eye, eye], dim=1).contiguous().to(dev)        # [64,128]
    bias = torch.zeros(2 * D, device=dev)
    zs = torch.zeros(2, 2 * D, device=dev)
    zs[1] = _pattern(MAGNITUDES, 2 * D).to(dev)
    zd = torch.zeros(2, 2 * D, device=dev)
    src = torch.zeros(E, dtype=torch.int32, device=dev)
    src[0] = 1
    src[-1] = 1
    dst = torch.zeros(E, dtype=torch.int32, device=dev)
    z = torch.full((E, 2 * D), -7.0, device=dev)
    h = torch.full((E, 2 * D), -7.0, device=dev)
    rc = lib.dm_edge_mlp3_f32(_fp(erow), _fp(wt), _fp(bias), _fp(zs), _fp(zd),
                              _ip(src), _ip(dst), _fp(z), _fp(h), E, D, 2 * D,
                              _stream())
    assert rc == 0, lib.dm_hip_last_error()
    # the planted values did arrive (the sign of a zero aside)
    want = zs[1].clone()
    assert bool(((z[0] == want) | (want == 0)).all())
    assert bool(((z[-1] == want) | (want == 0)).all())
    if E > 2:
        assert bool((z[1, :D] == erow[1]).all())
    _assert_same_bits(h, raw_act_eval(SILU, z, ref=True), f"h, E={E}")
    # and without z stored (another instantiation of the epilogue)
    h2 = torch.full((E, 2 * D), -7.0, device=dev)
    rc = lib.dm_edge_mlp3_f32(_fp(erow), _fp(wt), _fp(bias), _fp(zs), _fp(zd),
                              _ip(src), _ip(dst), None, _fp(h2), E, D, 2 * D,
                              _stream())
    assert rc == 0, lib.dm_hip_last_error()
    _assert_same_bits(h2, h, f"h without z, E={E}")


def _combine_ref(c, g, w, base):
    """base + ((c * sig(c)) * sig(g)) * w with the plain sigmoid, one rounding
    per operation."""
    from distmlip_amd.ops import raw_act_eval
    r = c * raw_act_eval(SIG, c.contiguous(), ref=True)
    r = r * raw_act_eval(SIG, g.contiguous(), ref=True)
    if w is not None:
        r = r * w
    if base is not None:
        r = r + base
    return r


@requires_gpu
@pytest.mark.parametrize("E", ROWS)
def test_tail_fwd_out_from_its_cg(E):
    """out of dm_gated_mlp_tail_fwd_f32 (keep form) from its own c|g.  Finite
    special values reach c and g through identity second-layer weights; the
    infinities through the bias of four columns."""
    from distmlip_amd.ops import _stream, hip_lib
    lib = hip_lib()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(601 + E)
    h = (3 * torch.randn(E, 2 * D, generator=gen)).to(dev)
    _plant(h[:, :D], FINITE)
    _plant(h[:, D:], FINITE, shift=7)
    w2 = torch.stack([torch.eye(D), torch.eye(D)]).contiguous().to(dev)
    b2 = torch.zeros(2, D, device=dev)
    inf = float("inf")
    b2[0, 60], b2[0, 61], b2[1, 62], b2[1, 63] = inf, -inf, inf, -inf
    w = torch.randn(E, D, generator=gen).to(dev)
    base = torch.randn(E, D, generator=gen).to(dev)
    cg = torch.full((2, E, D), -7.0, device=dev)
    out = torch.full((E, D), -7.0, device=dev)
    rc = lib.dm_gated_mlp_tail_fwd_f32(
        _fp(h), _fp(w2), _fp(w2, D * D), _fp(b2), _fp(b2, D), _fp(w),
        _fp(base), _fp(cg), _fp(cg, E * D), _fp(out), E, D, _stream())
    assert rc == 0, lib.dm_hip_last_error()
    # identity weights, zero bias: c|g are h's halves in the first 60 columns
    assert bool((cg[0][:, :60] == h[:, :60]).all())
    assert bool((cg[1][:, :60] == h[:, D:D + 60]).all())
    assert bool(cg[0][:, 60].isposinf().all() and cg[1][:, 63].isneginf().all())
    _assert_same_bits(out, _combine_ref(cg[0], cg[1], w, base),
                      f"out, E={E}")


@requires_gpu
@pytest.mark.parametrize("E", ROWS)
def test_tail_bwd_dw_from_c_g(E):
    """dw of dm_gated_mlp_tail_bwd_f32 (dense w): go * (c * sig(c)) * sig(g),
    with c and g given directly."""
    from distmlip_amd.ops import _stream, hip_lib, raw_act_eval
    lib = hip_lib()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(701 + E)
    c = _plant((3 * torch.randn(E, D, generator=gen)).to(dev), MAGNITUDES)
    g = _plant((3 * torch.randn(E, D, generator=gen)).to(dev), MAGNITUDES, 7)
    z = _plant((3 * torch.randn(E, 2 * D, generator=gen)).to(dev), MAGNITUDES)
    go = torch.randn(E, D, generator=gen).to(dev)
    w = torch.randn(E, D, generator=gen).to(dev)
    w2 = (torch.randn(2, D, D, generator=gen) / 8).to(dev)
    dz = torch.full((E, 2 * D), -7.0, device=dev)
    dw = torch.full((E, D), -7.0, device=dev)
    rc = lib.dm_gated_mlp_tail_bwd_f32(
        _fp(go), _fp(c), _fp(g), _fp(w), _fp(z), _fp(w2), _fp(w2, D * D),
        _fp(dz), _fp(dw), E, D, _stream())
    assert rc == 0, lib.dm_hip_last_error()
    silu_c = c * raw_act_eval(SIG, c, ref=True)
    want = (go * silu_c) * raw_act_eval(SIG, g, ref=True)
    _assert_same_bits(dw, want, f"dw, E={E}")
    assert not bool((dz == -7.0).any())


@requires_gpu
@pytest.mark.parametrize("E", ROWS)
def test_combine_fwd_and_silu_bwd(E):
    """out of dm_gated_combine_fwd_f32 and dz of dm_silu_bwd_f32 from the
    plain sigmoid.  k_silu_bwd contracts 1 + z (1 - s) into one fma: the
    product of two fp32 numbers is exact in fp64, so the fp64 sum rounded to
    fp32 is that fma (short of a double rounding, which needs an fp64 result
    exactly halfway between two fp32 numbers)."""
    from distmlip_amd.ops import _stream, hip_lib, raw_act_eval
    lib = hip_lib()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(801 + E)
    c = _plant((3 * torch.randn(E, D, generator=gen)).to(dev), MAGNITUDES)
    g = _plant((3 * torch.randn(E, D, generator=gen)).to(dev), MAGNITUDES, 7)
    w = torch.randn(E, D, generator=gen).to(dev)
    base = torch.randn(E, D, generator=gen).to(dev)
    out = torch.full((E, D), -7.0, device=dev)
    rc = lib.dm_gated_combine_fwd_f32(_fp(c), _fp(g), _fp(w), _fp(base),
                                      _fp(out), E * D, _stream())
    assert rc == 0, lib.dm_hip_last_error()
    _assert_same_bits(out, _combine_ref(c, g, w, base), f"combine, E={E}")

    z = _plant((3 * torch.randn(E, 2 * D, generator=gen)).to(dev), MAGNITUDES)
    go_h = torch.randn(E, 2 * D, generator=gen).to(dev)
    go_z = torch.randn(E, 2 * D, generator=gen).to(dev)
    dz = torch.full((E, 2 * D), -7.0, device=dev)
    rc = lib.dm_silu_bwd_f32(_fp(go_h), _fp(go_z), _fp(z), _fp(dz),
                             z.numel(), _stream())
    assert rc == 0, lib.dm_hip_last_error()
    s = raw_act_eval(SIG, z, ref=True)
    inner = (z.double() * (1.0 - s).double() + 1.0).float()
    want = go_h * (s * inner) + go_z
    _assert_same_bits(dz, want, f"silu_bwd, E={E}")
