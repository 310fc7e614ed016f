"""GPU tests of the first layer's reverse kernel in src-sorted row order with
the src segment sums of dz formed on chip (k_edge_mlp_bwd_src + k_seg_fixup,
entry point dm_edge_mlp_bwd_src_f32, HipOps.r_edge_mlp_bwd_src), against the
pair it replaces: dm_edge_mlp_bwd_f32 (or its patched form) followed by
dm_seg_sum_gather_f32 over the same dz.

ge must be the plain kernel's with torch.equal in every form (without gbase,
with it, out is gbase, patched).  The sums of a node whose sorted positions
lie within one 32-row tile must be the gather kernel's bits; over all elements
at most 1 fp32 ulp, the allowance of tests/test_gpu_fused_seg.py (a node over
several tiles gets its fp64 pieces added in tile order).  Against a torch fp64
index_add_ the sums hold one fp32 rounding plus the fp64 accumulation error
deg * sum|x| * 2^-52 of the two fp64 sums compared.

Block level: conv._AtomBlockFn on the graph of tests/test_gpu_atom_block.py
with and without DM_NO_FUSED_SRC_SEG=1: de and dbexp equal, dv within that
file's bound against fp64 plain torch.

DM_SRC_SEG_OUT=<file>: the measured figures are also written there as JSON."""
import json
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_mlp_tail_bwd import D, GUARD, SENTINEL, _bound  # noqa: E402
from test_gpu_fused_seg import _ordered  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs HIP GPU")

N = 37
E_CASES = [1, 31, 32, 33, 97, 4099]
EMPTY = (0, 18, 36)         # no rows: the first, a middle and the last node
M_PATCH = 5
FIGURES = {}


def _graph_of(src, dev):
    """perm (a stable sort of the rows by src: random rows, sorted nodes),
    seg = src[perm], row_ptr."""
    E = len(src)
    perm = torch.argsort(src, stable=True)
    rp = torch.zeros(N + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(torch.bincount(src, minlength=N), 0)
    return types.SimpleNamespace(
        E=E, src=src.to(dev), perm=perm.to(torch.int32).to(dev),
        seg=src[perm].to(torch.int32).to(dev),
        row_ptr=rp.to(torch.int32).to(dev), rp=rp)


def _graphs(dev):
    gen = torch.Generator().manual_seed(90210)
    live = torch.tensor([n for n in range(N) if n not in EMPTY])
    gs = {}
    for E in E_CASES:
        src = live[torch.randint(0, len(live), (E,), generator=gen)]
        gs[f"E{E}"] = _graph_of(src, dev)
    # planted: node 1 fills tile 0 exactly (a segment boundary on the tile
    # boundary), node 3 has 70 rows at positions 42..111 (tiles 1, 2 and 3),
    # empty nodes first, in the middle and last, a ragged last tile
    deg = torch.zeros(N, dtype=torch.int64)
    deg[1], deg[2], deg[3], deg[5], deg[20], deg[35] = 32, 10, 70, 5, 33, 3
    src = torch.repeat_interleave(torch.arange(N), deg)
    gs["planted"] = _graph_of(src[torch.randperm(len(src), generator=gen)],
                              dev)
    assert gs["planted"].rp[2] == 32 and gs["planted"].rp[3] == 42
    gs["one_node"] = _graph_of(torch.full((97,), 5, dtype=torch.int64), dev)
    return gs


GRAPH_NAMES = [f"E{E}" for E in E_CASES] + ["planted", "one_node"]


class _Data:
    def __init__(self):
        self.dev = dev = torch.device("cuda:0")
        self.graphs = _graphs(dev)
        E = max(E_CASES)
        gen = torch.Generator(device="cpu").manual_seed(1618)
        self.dz = torch.randn(E, 2 * D, generator=gen).to(dev)
        self.gbase = torch.randn(E, D, generator=gen).to(dev)
        self.wt = (torch.randn(D, 2 * D, generator=gen) / 8).to(dev)
        self.rows = torch.randn(M_PATCH + 2, D, generator=gen).to(dev)


@pytest.fixture(scope="module")
def data():
    d = _Data()
    yield d
    path = os.environ.get("DM_SRC_SEG_OUT")
    if path and FIGURES:
        with open(path, "w") as f:
            json.dump(FIGURES, f, indent=1)
            f.write("\n")


def _guarded(dev, E):
    buf = torch.full((2 * GUARD + E * D,), SENTINEL, device=dev)
    return buf, buf[GUARD:GUARD + E * D].view(E, D)


def _check_guards(buf, E, what):
    n = E * D
    assert bool((buf[:GUARD] == SENTINEL).all()), f"{what}: front guard"
    assert bool((buf[GUARD + n:] == SENTINEL).all()), f"{what}: rear guard"
    assert not bool((buf[GUARD:GUARD + n] == SENTINEL).any()), \
        f"{what}: elements left unwritten"


def _check_sums(sums, dz, g, what):
    from distmlip_amd.ops import raw_seg_sum_gather
    pair = raw_seg_sum_gather(dz, g.perm, g.row_ptr, N)
    off = (_ordered(sums) - _ordered(pair)).abs()
    share = (off > 0).double().mean().item()
    # nodes whose positions lie in one tile: the gather kernel's bits
    lo, hi = g.rp[:-1], g.rp[1:]
    one_tile = ((hi == lo) | ((lo >> 5) == ((hi - 1) >> 5))).to(dz.device)
    assert torch.equal(sums[one_tile], pair[one_tile]), \
        f"{what}: a node within one tile differs from the gather kernel"
    assert int(off.max()) <= 1, f"{what}: {int(off.max())} ulp from the pair"
    assert not sums[(hi == lo).to(dz.device)].any(), \
        f"{what}: a node without rows is not 0"
    # fp64 reference: one fp32 rounding + the accumulation error of two fp64
    # sums of deg terms
    ref = torch.zeros(N, 2 * D, dtype=torch.float64, device=dz.device)
    ref.index_add_(0, g.src, dz.double())
    mag = torch.zeros_like(ref).index_add_(0, g.src, dz.double().abs())
    r32 = ref.float().abs()
    spacing = (torch.nextafter(r32, torch.full_like(r32, float("inf")))
               - r32).double()
    deg = (hi - lo).double().to(dz.device)[:, None]
    tol = 0.5 * spacing + deg * mag * 2.0 ** -52
    err = (sums.double() - ref).abs()
    worst = (err / spacing).max().item()
    print(f"{what}: E={g.E} differ {share:.3e} of elements, max "
          f"{int(off.max())} ulp from the pair; vs fp64 {worst:.3f} ulp")
    FIGURES[what] = {"E": g.E, "share_differing": share,
                     "max_ulp_from_pair": int(off.max()),
                     "max_ulp_from_fp64": worst}
    assert bool((err <= tol).all()), f"{what}: {worst} ulp from fp64"


@requires_gpu
@pytest.mark.parametrize("name", GRAPH_NAMES)
def test_ge_and_sums(data, name):
    from distmlip_amd.ops import raw_edge_mlp_bwd, raw_edge_mlp_bwd_src
    d, g = data, data.graphs[name]
    E = g.E
    dz, gbase = d.dz[:E].contiguous(), d.gbase[:E].contiguous()
    dz0, gbase0 = dz.clone(), gbase.clone()
    order = (g.perm, g.seg, g.row_ptr)
    # without gbase
    buf, out = _guarded(d.dev, E)
    ge, sums = raw_edge_mlp_bwd_src(dz, d.wt, *order, None, out)
    torch.cuda.synchronize()
    _check_guards(buf, E, name)
    assert ge is out and torch.equal(ge, raw_edge_mlp_bwd(dz, d.wt))
    _check_sums(sums, dz, g, f"{name} plain")
    # with gbase, a fresh out
    want = raw_edge_mlp_bwd(dz, d.wt, gbase)
    buf, out = _guarded(d.dev, E)
    ge, sums_b = raw_edge_mlp_bwd_src(dz, d.wt, *order, gbase, out)
    torch.cuda.synchronize()
    _check_guards(buf, E, name)
    assert torch.equal(ge, want), f"{name}: gbase"
    assert torch.equal(sums_b, sums)
    # out is gbase
    buf, own = _guarded(d.dev, E)
    own.copy_(gbase)
    ge, sums_i = raw_edge_mlp_bwd_src(dz, d.wt, *order, own, own)
    torch.cuda.synchronize()
    _check_guards(buf, E, name)
    assert ge is own and torch.equal(own, want), f"{name}: in place"
    assert torch.equal(sums_i, sums)
    # patched: M rows, the rows of the last sorted positions (the ragged
    # last tile) among them
    M = min(M_PATCH, E)
    rows = torch.cat([g.perm[E - (M + 1) // 2:].long(),
                      g.perm[:M // 2].long()])
    assert len(rows) == M
    slot = torch.full((E,), -1, dtype=torch.int32, device=d.dev)
    slot[rows] = torch.arange(M, dtype=torch.int32, device=d.dev) + 1
    want_p = raw_edge_mlp_bwd(dz, d.wt, gbase, patch=(slot, d.rows))
    ge, sums_p = raw_edge_mlp_bwd_src(dz, d.wt, *order, gbase,
                                      patch=(slot, d.rows))
    assert torch.equal(ge, want_p), f"{name}: patched"
    assert torch.equal(sums_p, sums)
    own = gbase.clone()
    raw_edge_mlp_bwd_src(dz, d.wt, *order, own, own, patch=(slot, d.rows))
    assert torch.equal(own, want_p), f"{name}: patched in place"
    assert torch.equal(dz, dz0) and torch.equal(gbase, gbase0), \
        "an input was written to"


@requires_gpu
def test_entry_refusals(data):
    import ctypes
    from distmlip_amd.ops import _fp, _ip, _stream, hip_lib
    d, g = data, data.graphs["E97"]
    E = g.E
    buf, out = _guarded(d.dev, E)
    sums = torch.full((N, 2 * D), SENTINEL, device=d.dev)
    part = torch.empty(4, 2, 2 * D, dtype=torch.float64, device=d.dev)
    pp = ctypes.cast(part.data_ptr(), ctypes.POINTER(ctypes.c_double))
    slot = torch.full((E,), -1, dtype=torch.int32, device=d.dev)

    def entry(gbase=_fp(d.gbase), slot_=None, patch=None, out_=_fp(out),
              perm=_ip(g.perm), seg=_ip(g.seg), rp=_ip(g.row_ptr),
              sums_=_fp(sums), part_=pp, din=2 * D, dout=D):
        return hip_lib().dm_edge_mlp_bwd_src_f32(
            _fp(d.dz), _fp(d.wt), gbase, slot_, patch, out_, perm, seg, rp,
            sums_, part_, E, N, din, dout, _stream())

    assert entry(din=64) != 0 and entry(dout=32) != 0
    for k in ("out_", "perm", "seg", "rp", "sums_", "part_"):
        assert entry(**{k: None}) != 0, k
    assert entry(gbase=None, slot_=_ip(slot)) != 0     # a patch needs a gbase
    assert entry(slot_=_ip(slot), patch=_fp(out)) != 0       # patch is out
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()) and bool((sums == SENTINEL).all()), \
        "a refused call launched"


@requires_gpu
def test_hipops_atom_and_line():
    """HipOps.r_edge_mlp_bwd_src on a graph object: the atom graph's src
    order and, with line=True, the line graph's."""
    from distmlip_amd.ops import HipOps
    from test_gpu_mlp_tail_bwd import E_SMALL, _graphs as _pd_graphs
    dev = torch.device("cuda:0")
    pd, _ = _pd_graphs(dev)
    ops = HipOps()
    gen = torch.Generator(device="cpu").manual_seed(33)
    dz = torch.randn(E_SMALL, 2 * D, generator=gen).to(dev)
    gbase = torch.randn(E_SMALL, D, generator=gen).to(dev)
    wt = (torch.randn(D, 2 * D, generator=gen) / 8).to(dev)
    for line, seg_of in ((False, ops.r_seg_src), (True, ops.r_seg_lsrc)):
        ge, ss = ops.r_edge_mlp_bwd_src(dz, wt, gbase, pd, line=line)
        assert torch.equal(ge, ops.r_edge_mlp_bwd(dz, wt, gbase))
        pair = seg_of(dz, pd)
        assert ss.shape == pair.shape
        assert int((_ordered(ss) - _ordered(pair)).abs().max()) <= 1


@requires_gpu
@pytest.mark.parametrize("masked", [False, True])
def test_block_with_and_without_the_switch(monkeypatch, masked):
    from distmlip_amd import mlp_path
    from distmlip_amd.ops import HipOps
    from oracle.chgnet_ref import CpuRefOps
    from test_gpu_atom_block import NAMES, _Case, _run
    from test_gpu_mlp_tail_bwd import _graphs as _pd_graphs
    dev = torch.device("cuda:0")
    pd, pr = _pd_graphs(dev)
    case = _Case(dev)
    monkeypatch.delenv(mlp_path.NO_FUSED_SRC_SEG, raising=False)
    launches = []
    real = HipOps.r_edge_mlp_bwd_src

    def counted(self, *a, **k):
        launches.append(1)
        return real(self, *a, **k)

    monkeypatch.setattr(HipOps, "r_edge_mlp_bwd_src", counted)
    assert mlp_path.fused_src_seg(HipOps(), D)
    new = _run(case, pd, HipOps(), torch.float32, "block", 2, masked, True)
    assert len(launches) == 4, "two first-layer reverses per block"
    monkeypatch.setenv(mlp_path.NO_FUSED_SRC_SEG, "1")
    assert not mlp_path.fused_src_seg(HipOps(), D)
    old = _run(case, pd, HipOps(), torch.float32, "block", 2, masked, True)
    assert len(launches) == 4, "the switch did not restore r_seg_src"
    ref = _run(case, pr, CpuRefOps(), torch.float64, "plain", 2, masked, True)
    got = dict(zip(NAMES, new))
    was = dict(zip(NAMES, old))
    for name in ("v2", "e2"):
        assert torch.equal(got[name], was[name]), name
    for name, r in zip(NAMES, ref):
        _bound(got[name], r, was[name], f"{name} mask={masked}")
    # one block (its e gradient and dbexp read no segment sum of its own dz)
    monkeypatch.delenv(mlp_path.NO_FUSED_SRC_SEG)
    new1 = dict(zip(NAMES, _run(case, pd, HipOps(), torch.float32, "block", 1,
                                masked, True)))
    monkeypatch.setenv(mlp_path.NO_FUSED_SRC_SEG, "1")
    old1 = dict(zip(NAMES, _run(case, pd, HipOps(), torch.float32, "block",
                                1, masked, True)))
    for name in ("de", "dbexp"):
        assert torch.equal(new1[name], old1[name]), name
