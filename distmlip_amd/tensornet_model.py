"""TensorNet model restatement — weights container + architecture metadata.

The reference distributes matgl's TensorNet
(implementations/matgl/models/tensornet.py: per-partition embedding,
interaction layers with `atom_transfer` between them, aggregate, readout)
and delegates all of its arithmetic to matgl, which is not installable
here.  As with CHGNet (distmlip_amd/model.py) and MACE
(distmlip_amd/mace_model.py) this is a from-scratch restatement of the
published architecture (Simeon & De Fabritiis, "TensorNet: Cartesian
tensor representations for efficient learning of molecular potentials",
NeurIPS 2023, as matgl implements it); the forwards live in
distmlip_amd/tensornet_ops.py and are shared by both drivers
(tensornet.TensorNet_Dist, tensornet_runtime.TensorNetSpmdEngine).

Node state: one 3x3 tensor per channel, X[n, c, 3, 3] in matgl.  The
product stores it component-major, X[n, 3a+b, c], so that one node's
channels are one contiguous 256 B row per tensor component at units = 64
(lane = channel in the fused message kernel).

Row order of the two ->3C linears (`TensorEmbedding.scalar2` and
`Interaction.edge3`): matgl reshapes their output as (-1, C, 3), i.e. output
row c*3 + k belongs to channel c and part k in (I, A, S).  The product reads
the same output as [*, 3, C] (row k*C + c), so this container holds those
two weights with their rows in k-major order.  `kmajor_rows(C)` is the
permutation that converts a matgl weight: W_here = W_matgl[kmajor_rows(C)]
(and the same for the bias); INTEGRATION.md lists it with the rest of the
mapping.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
from torch import nn


@dataclass
class TensorNetConfig:
    n_elements: int
    units: int = 64
    nblocks: int = 2
    num_rbf: int = 32
    cutoff: float = 5.0
    rbf_width: Optional[float] = None      # default (num_rbf - 1) / cutoff
    group: str = "O(3)"                    # or "SO(3)"
    is_intensive: bool = False
    data_mean: float = 0.0
    data_std: float = 1.0

    def __post_init__(self):
        if self.rbf_width is None:
            self.rbf_width = (self.num_rbf - 1) / self.cutoff
        if self.group not in ("O(3)", "SO(3)"):
            raise ValueError(f"group must be 'O(3)' or 'SO(3)', "
                             f"got {self.group!r}")


def kmajor_rows(C: int) -> torch.Tensor:
    """Row permutation from matgl's channel-major (c*3 + k) output order of
    a ->3C linear to the k-major (k*C + c) order stored here."""
    k = torch.arange(3).repeat_interleave(C)
    c = torch.arange(C).repeat(3)
    return c * 3 + k


class TensorEmbedding(nn.Module):
    """matgl TensorEmbedding restatement (weights only)."""

    def __init__(self, cfg: TensorNetConfig):
        super().__init__()
        C, R = cfg.units, cfg.num_rbf
        self.emb = nn.Embedding(cfg.n_elements, C)
        self.pair = nn.Linear(2 * C, C)                 # Z_e
        self.rbf_I = nn.Linear(R, C)                    # W_1
        self.rbf_A = nn.Linear(R, C)                    # W_2
        self.rbf_S = nn.Linear(R, C)                    # W_3
        self.norm = nn.LayerNorm(C)
        self.mix = nn.ModuleList(
            [nn.Linear(C, C, bias=False) for _ in range(3)])
        self.scalar1 = nn.Linear(C, 2 * C)
        self.scalar2 = nn.Linear(2 * C, 3 * C)          # rows k-major


class Interaction(nn.Module):
    """matgl TensorNetInteraction restatement (weights only)."""

    def __init__(self, cfg: TensorNetConfig):
        super().__init__()
        C, R = cfg.units, cfg.num_rbf
        self.edge1 = nn.Linear(R, C)
        self.edge2 = nn.Linear(C, 2 * C)
        self.edge3 = nn.Linear(2 * C, 3 * C)            # rows k-major
        self.mix = nn.ModuleList(
            [nn.Linear(C, C, bias=False) for _ in range(6)])


class TensorNetCore(nn.Module):
    """All learnable state of the TensorNet restatement."""

    def __init__(self, config: TensorNetConfig):
        super().__init__()
        cfg = config
        self.config = cfg
        C = cfg.units
        self.embedding = TensorEmbedding(cfg)
        self.layers = nn.ModuleList(
            [Interaction(cfg) for _ in range(cfg.nblocks)])
        self.out_norm = nn.LayerNorm(3 * C)
        self.linear = nn.Linear(3 * C, C)
        self.final_layer = nn.Sequential(
            nn.Linear(C, C), nn.SiLU(), nn.Linear(C, C), nn.SiLU(),
            nn.Linear(C, 1))
        self.register_buffer("data_mean", torch.tensor(cfg.data_mean))
        self.register_buffer("data_std", torch.tensor(cfg.data_std))
        # per-element energy references (matgl AtomRef analog, applied by
        # Potential_Dist as the reference's pes.py:111-113 does)
        self.element_refs = nn.Parameter(torch.zeros(cfg.n_elements))

    @classmethod
    def seeded(cls, config: TensorNetConfig, seed: int = 0,
               dtype: torch.dtype = torch.float32) -> "TensorNetCore":
        """Deterministic weights with torch's default layer initialisation
        (what an untrained matgl TensorNet holds)."""
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            core = cls(config)
            with torch.no_grad():
                core.element_refs.normal_(0.0, 0.1)
        return core.to(dtype)
