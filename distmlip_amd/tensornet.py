"""TensorNet_Dist — the distributed TensorNet forward (drop-in model class).

API mirror of the reference adapter
implementations/matgl/models/tensornet.py (TensorNet_Dist):
`from_existing` (tensornet.py:204-214), `enable_distributed_mode`
(tensornet.py:164-202), `potential_forward_dist` (tensornet.py:10-117)
returning (node_types, positions, strain, (total_E, None)), `dist_forward`
(tensornet.py:119-161: interaction layers with `atom_transfer` between
them, aggregate, decompose / norm / readout, `is_intensive` refused) and
`predict_structure_dist` (tensornet.py:216-232, refused) — re-implemented
over this package's from-scratch TensorNet restatement (tensornet_model /
tensornet_ops) instead of DGL/matgl.

Single-process mode: a list of per-partition devices exactly like the
reference ("cpu" entries allowed); halo = differentiable slice copies.  The
SPMD production engine (one process per GPU over RCCL) is
distmlip_amd/tensornet_runtime.TensorNetSpmdEngine; both run the same
embedding and layer body (tensornet_ops).

Divergence: the embedding sums over a node's in-edges, which a partition
holds for the nodes it owns only (edges belong to their dst's partition),
so the ghosts' rows are exchanged once after the embedding as well as after
every layer.  Without it the first layer would read incomplete ghost
tensors and the result would depend on the partition count.
"""
from __future__ import annotations

from copy import deepcopy

import numpy as np
import torch

from distmlip_amd import tensornet_ops as tno
from distmlip_amd.chgnet import PartitionData
from distmlip_amd.ops_base import default_ops_factory
from distmlip_amd.tensornet_model import TensorNetCore


class TensorNet_Dist(torch.nn.Module):
    """Distributed TensorNet model (drop-in for the reference class)."""

    __version__ = 1

    def __init__(self, core: TensorNetCore):
        super().__init__()
        self.core = core
        self.config = core.config
        self.dist_enabled = False
        self.use_bond_graph = False
        self.cutoff = core.config.cutoff
        self.three_body_cutoff = 0.0

    # -- reference surface -------------------------------------------------

    @classmethod
    def from_existing(cls, model, dtype=None):
        """Wrap an existing TensorNetCore (reference tensornet.py:204-214).
        INTEGRATION.md documents the weight mapping a matgl TensorNet
        converts through."""
        core = model.core if isinstance(model, TensorNet_Dist) else model
        m = cls(deepcopy(core).to("cpu"))
        if dtype is not None:
            m.core = m.core.to(dtype)
        return m

    def enable_distributed_mode(self, gpus, ops_factory=None):
        """Replicate weights per device (reference tensornet.py:164-202).
        `gpus`: ints (cuda ordinals) and/or "cpu"; `ops_factory` maps device
        -> OpsBackend, default the HIP product backend (GPU only)."""
        if self.dist_enabled:
            raise Exception(
                "Current model already has distributed mode enabled.")
        self.gpus = ["cpu" if g == "cpu" else f"cuda:{g}" for g in gpus]
        factory = ops_factory or default_ops_factory
        self.cores = [deepcopy(self.core).to(dev).eval()
                      for dev in self.gpus]
        for c in self.cores:
            c.requires_grad_(False)
        self.ops = [factory(torch.device(dev)) for dev in self.gpus]
        self.dist_enabled = True

    def set_local_species(self, dist_info, species: np.ndarray):
        self._local_species = []
        for p in range(dist_info.num_partitions):
            ids = np.asarray(dist_info.global_ids[p])
            self._local_species.append(
                torch.as_tensor(np.asarray(species)[ids], dtype=torch.long)
                .to(self.gpus[p]))

    def predict_structure_dist(self, structure, state_feats=None):
        raise NotImplementedError(
            "Distributed direct property prediction is not yet supported. "
            "Please use Potential_Dist")

    # -- forward -----------------------------------------------------------

    def potential_forward_dist(self, dist_info, structure, lattice_matrix,
                               calc_stresses, calc_forces, calc_hessian,
                               state_attr=None):
        """Reference tensornet.py:10-117 flow (single process, P
        partitions): global geometry on the root device, distributed per
        partition, per-partition embedding, then dist_forward."""
        assert self.dist_enabled
        ft = next(self.core.parameters()).dtype
        root = self.gpus[0]
        P = dist_info.num_partitions

        lattice0 = torch.tensor(np.asarray(lattice_matrix), dtype=ft,
                                device=root)
        strain = lattice0.new_zeros(3, 3)
        if calc_stresses:
            strain.requires_grad_(True)
        lattice = lattice0 @ (torch.eye(3, device=root, dtype=ft) + strain)
        frac = torch.tensor(np.asarray(structure.frac_coords), dtype=ft,
                            device=root)
        pos_global = frac @ lattice
        if calc_forces:
            pos_global.requires_grad_(True)
            pos_global.retain_grad()
        node_types = torch.tensor(np.asarray(structure.species),
                                  dtype=torch.long, device=root)

        idx1 = torch.as_tensor(dist_info.py_index_1, dtype=torch.long).to(root)
        idx2 = torch.as_tensor(dist_info.py_index_2, dtype=torch.long).to(root)
        off = torch.tensor(np.asarray(dist_info.py_offsets), dtype=ft,
                           device=root)
        big_bond_vec = pos_global[idx2] + off @ lattice - pos_global[idx1]

        parts, geom, X = [], [], []
        for p in range(P):
            pd = PartitionData(dist_info, p, self.gpus[p], False)
            vec = dist_info.global_to_local_edges(big_bond_vec, p,
                                                  self.gpus[p])
            g = tno.edge_basis(vec, self.cores[p])
            parts.append(pd)
            geom.append(g)
            X.append(tno.tn_embedding(self.cores[p], self._local_species[p],
                                      *g, pd, self.ops[p]))
        return (node_types, pos_global, strain,
                (self.dist_forward(parts, geom, X, dist_info), None))

    def dist_forward(self, parts, geom, X, dist_info):
        """Reference tensornet.py:119-161 flow over the ops backend."""
        P = dist_info.num_partitions
        C = self.config.units

        def transfer(X):
            flat = dist_info.atom_transfer(
                [x.reshape(x.shape[0], 9 * C) for x in X])
            return [x.view(-1, 9, C) for x in flat]

        X = transfer(X)          # ghosts' embedding rows (module docstring)
        for i in range(self.config.nblocks):
            for p in range(P):
                _, rbf, cut = geom[p]
                X[p] = tno.tn_layer(self.cores[p].layers[i], X[p], rbf, cut,
                                    parts[p], self.ops[p], self.config.group)
            X = transfer(X)      # tensornet.py:128
        Xa = dist_info.aggregate(X, device=self.gpus[0])
        return tno.tn_node_energy(self.cores[0], Xa).sum()
