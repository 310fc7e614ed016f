"""GPU tests of the dense w read through a row index (w_idx) in the gated-MLP
kernels: dm_gated_mlp_tail_fwd_widx_f32, dm_gated_mlp4_widx_f32 and
dm_gated_mlp_tail_bwd_widx_f32.  Each indexed form against the plain form on
the materialized w[w_idx]; every output torch.equal.

Rows 1, 31, 32, 33 (tile tails), 4099 (more than one block; every wave still
takes one tile) and 98304 + 33: above both grid caps (512 blocks x 4 waves x
32 rows = 65536 for the whole-MLP kernel, 768 x 4 x 32 = 98304 for the two
tail kernels), so waves walk a second tile with the index loaded per tile,
the last tile is a tail, and the whole-MLP kernel loads its index next to the
prefetch of the following tile.  A w table of 257 rows; an index with repeats
that names the first and the last table row (at one row: the last)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_fused_seg import _graph  # noqa: E402

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs HIP GPU")

D = 64
T = 257
N_TAB = 61                  # rows of the three gathered first-layer tables
E_ABOVE_CAPS = 98304 + 33
ROWS = [1, 31, 32, 33, 4099, E_ABOVE_CAPS]


class _Data:
    def __init__(self):
        self.dev = dev = torch.device("cuda:0")
        gen = torch.Generator(device="cpu").manual_seed(1618)
        E = max(ROWS)

        def rnd(*shape):
            return torch.randn(*shape, generator=gen).to(dev)

        def idx(n):
            return torch.randint(0, n, (E,), generator=gen).to(
                torch.int32).to(dev)

        self.w_tab = rnd(T, D)
        self.w_idx_all = idx(T)
        self.h, self.base = rnd(E, 2 * D), rnd(E, D)
        self.w2, self.b2 = rnd(2, D, D) / 8, rnd(2, 1, D)
        self.row, self.wt, self.bias = rnd(E, D), rnd(D, 2 * D) / 8, rnd(2 * D)
        self.tables = tuple(rnd(N_TAB, 2 * D) for _ in range(3))
        self.idx3 = tuple(idx(N_TAB) for _ in range(3))
        self.go, self.cg, self.z = rnd(E, D), rnd(2, E, D), rnd(E, 2 * D)
        self.go_tab, self.go_idx = rnd(300, D), idx(300)

    def w_idx(self, E):
        """E indices into the table: repeats, the first and the last row."""
        i = self.w_idx_all[:E].clone()
        if E >= 3:
            i[1] = i[2]
        i[0] = 0
        i[E - 1] = T - 1
        assert E < 3 or (len(torch.unique(i)) < E and int(i.min()) == 0)
        assert int(i.max()) == T - 1
        return i


@pytest.fixture(scope="module")
def data():
    return _Data()


def _same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), f"{what}: output {k}"
        if g is not None:
            assert torch.equal(g, w), f"{what}: output {k} differs"


@requires_gpu
@pytest.mark.parametrize("E", ROWS)
@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("with_base", [False, True])
def test_tail_fwd(data, with_base, keep, E):
    from distmlip_amd.ops import raw_mlp_tail_fwd
    d, i = data, data.w_idx(E)
    base = d.base[:E] if with_base else None
    args = (d.h[:E], d.w2, d.b2)
    want = raw_mlp_tail_fwd(*args, d.w_tab[i.long()], base, keep)
    got = raw_mlp_tail_fwd(*args, d.w_tab, base, keep, w_idx=i)
    _same(got, want, f"tail fwd keep={keep} base={with_base} E={E}")


@requires_gpu
@pytest.mark.parametrize("E", ROWS)
@pytest.mark.parametrize("keep", [False, True])
def test_whole_mlp(data, keep, E):
    from distmlip_amd.ops import raw_gated_mlp
    d, i = data, data.w_idx(E)
    args = (d.row[:E], d.wt, d.bias, d.tables,
            tuple(x[:E].contiguous() for x in d.idx3), d.w2, d.b2)
    want = raw_gated_mlp(*args, d.w_tab[i.long()], None, keep)
    got = raw_gated_mlp(*args, d.w_tab, None, keep, w_idx=i)
    _same(got, want, f"whole MLP keep={keep} E={E}")


@requires_gpu
@pytest.mark.parametrize("E", ROWS)
@pytest.mark.parametrize("seg", [False, True])
@pytest.mark.parametrize("indexed", [False, True])
def test_tail_bwd(data, indexed, seg, E):
    from distmlip_amd.ops import raw_mlp_tail_bwd
    d, i = data, data.w_idx(E)
    go, go_idx = (d.go_tab, d.go_idx[:E].contiguous()) if indexed \
        else (d.go[:E], None)
    g = _graph([0, 3, 40, 0, 70] + [200] * 500, d.dev, E) if seg else None
    cg = d.cg[:, :E].contiguous()
    want = raw_mlp_tail_bwd(go, cg, d.w_tab[i.long()], d.z[:E], d.w2, go_idx,
                            seg=g)
    got = raw_mlp_tail_bwd(go, cg, d.w_tab, d.z[:E], d.w2, go_idx, seg=g,
                           w_idx=i)
    assert got[1].shape == (E, D)
    _same(got, want, f"tail bwd idx={indexed} seg={seg} E={E}")


@requires_gpu
def test_forms_refused(data):
    """The whole-MLP kernel takes w_idx without base only, and not in its
    two-gather form."""
    from distmlip_amd.ops import raw_gated_mlp
    d, E = data, 33
    i = d.w_idx(E)
    idx3 = tuple(x[:E].contiguous() for x in d.idx3)
    with pytest.raises(AssertionError):
        raw_gated_mlp(d.row[:E], d.wt, d.bias, d.tables, idx3, d.w2, d.b2,
                      d.w_tab, d.base[:E], False, w_idx=i)
    with pytest.raises(AssertionError):
        raw_gated_mlp(d.row[:E], d.wt, d.bias, d.tables[:2], idx3[:2], d.w2,
                      d.b2, d.w_tab, None, False, w_idx=i)
