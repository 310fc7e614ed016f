"""The switch table of distmlip_amd.mlp_path: what each A/B switch, set
alone, turns off; and that the lean forwards of conv.py honour
DM_NO_FUSED_MLP like chgnet.gated_mlp_split3/4 do."""
import types

import pytest
import torch

from distmlip_amd import conv, mlp_path as mp
from distmlip_amd.ops import HipOps
from oracle.chgnet_ref import CpuRefOps

PREDICATES = {
    "first": lambda o, d: mp.fused_first(o, d),
    "first4": lambda o, d: mp.fused_first(o, d, "edge_mlp4_act"),
    "first_raw": lambda o, d: mp.fused_first(o, d, "r_edge_mlp3"),
    "first_bwd": lambda o, d: mp.fused_first_bwd(o, d),
    "tail_fwd": lambda o, d: mp.fused_tail_fwd(o, d),
    "tail_act": lambda o, d: mp.fused_tail_fwd(o, d, "mlp_tail_act"),
    "tail_bwd": lambda o, d: mp.fused_tail_bwd(o, d),
    "tail_node": lambda o, d: mp.fused_tail_bwd(o, d, "mlp_tail"),
    "tail_idx": lambda o, d: mp.indexed_tail_bwd(o, d),
    "whole_keep": lambda o, d: mp.whole_mlp_keep(o, d),
    "whole_act": lambda o, d: mp.whole_mlp_act(o, d),
    "factored": lambda o, d: mp.factored_w(o, d),
    "keep_packs": lambda o, d: mp.fused_keep_packs(),
    "atom_block": lambda o, d: mp.atom_block(o, d),
    "final_keep": lambda o, d: mp.final_keep(),
    "row_exchange": lambda o, d: mp.row_exchange(),
    "native_rows": lambda o, d: mp.native_rows(o),
    "fused_conv": lambda o, d: mp.fused_conv(o),
    "fused_conv4": lambda o, d: mp.fused_conv(o, "r_gather_add4"),
    "whole_graph": lambda o, d: mp.whole_graph(o),
    "whole_graph_ckpt": lambda o, d: mp.whole_graph_ckpt(),
}
OFF_BY_DEFAULT = {"fused_conv", "fused_conv4", "whole_graph_ckpt"}

# switch=value -> the predicates that flip against the default, HipOps, d=64
FLIPS = {
    "DM_NO_FUSED_MLP=1": {"first", "first4", "first_raw", "whole_keep",
                          "whole_act", "atom_block"},
    "DM_FUSED_MLP=1": set(),
    "DM_NO_FUSED_MLP_BWD=1": {"tail_bwd", "tail_node", "tail_idx",
                              "factored"},
    "DM_NO_FUSED_MLP_FWD=1": {"tail_fwd", "tail_act", "whole_keep",
                              "whole_act", "factored"},
    "DM_NO_FUSED_MLP1_BWD=1": {"first_bwd"},
    "DM_NO_FUSED_MLP_FULL=1": {"whole_keep", "whole_act"},
    "DM_NO_FACTORED_W=1": {"factored"},
    "DM_NO_ATOM_BLOCK=1": {"atom_block", "keep_packs"},
    "DM_NO_FINAL_KEEP=1": {"final_keep"},
    "DM_NO_ROW_EXCHANGE=1": {"row_exchange"},
    "DM_FUSED_CONV=1": {"fused_conv", "fused_conv4", "atom_block"},
    "DM_WHOLE_GRAPH=0": {"whole_graph"},
    "DM_WHOLE_GRAPH_CKPT=1": {"whole_graph_ckpt", "row_exchange"},
}


@pytest.fixture
def clean_env(monkeypatch):
    for name in mp.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def _state(ops, d):
    return {k: bool(f(ops, d)) for k, f in PREDICATES.items()}


def test_every_switch_is_listed():
    assert {s.split("=")[0] for s in FLIPS} == set(mp.SWITCHES)


def test_defaults(clean_env):
    hip = _state(HipOps, 64)
    assert {k for k, v in hip.items() if not v} == OFF_BY_DEFAULT
    # another width: no kernel path, the step-level policies stay
    assert {k for k, v in _state(HipOps, 32).items() if v} == {
        "keep_packs", "final_keep", "row_exchange", "native_rows",
        "whole_graph"}
    # the fp64 reference backend has the autograd first layers only
    assert {k for k, v in _state(CpuRefOps(), 64).items() if v} == {
        "first", "first4", "keep_packs", "final_keep", "row_exchange",
        "whole_graph"}


@pytest.mark.parametrize("setting", sorted(FLIPS))
def test_switch_alone(clean_env, setting):
    default = _state(HipOps, 64)
    name, value = setting.split("=")
    clean_env.setenv(name, value)       # read at call time, nothing cached
    got = _state(HipOps, 64)
    assert {k for k in got if got[k] != default[k]} == FLIPS[setting]
    clean_env.delenv(name)
    assert _state(HipOps, 64) == default


class _Counting(CpuRefOps):
    def __init__(self):
        self.calls = []

    def edge_mlp3_act(self, *a):
        self.calls.append("edge_mlp3_act")
        return super().edge_mlp3_act(*a)

    def gather_add3_act(self, *a):
        self.calls.append("gather_add3_act")
        return super().gather_add3_act(*a)


def test_lean_atom_honours_no_fused_mlp(clean_env):
    d, n_atoms = 64, 3
    g = torch.Generator().manual_seed(0)

    def rnd(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    pd = types.SimpleNamespace(src=torch.tensor([0, 1, 2, 0]),
                               dst=torch.tensor([1, 2, 0, 2]),
                               n_atoms=n_atoms)

    def pack():
        wcg = rnd(2 * d, 3 * d) / 8
        return (wcg, rnd(2 * d), rnd(2, d, d) / 8, rnd(2, 1, d),
                wcg[:, 2 * d:].t().contiguous())

    pe, pn = pack(), pack()
    args = (pd, rnd(n_atoms, d), rnd(4, d), rnd(4, d), rnd(4, d), pe, pn, d)
    fused, plain = _Counting(), _Counting()
    with torch.no_grad():
        v_f, e_f = conv._lean_atom(fused, *args)
        clean_env.setenv("DM_NO_FUSED_MLP", "1")
        v_p, e_p = conv._lean_atom(plain, *args)
    assert fused.calls == ["edge_mlp3_act"] * 2
    assert plain.calls == ["gather_add3_act"] * 2
    torch.testing.assert_close(v_p, v_f, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(e_p, e_f, rtol=1e-12, atol=1e-12)
