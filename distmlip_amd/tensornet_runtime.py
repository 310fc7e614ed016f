"""TensorNet SPMD runtime — one process per GPU over torch.distributed.

MI355X-native replacement for the reference's single-process TensorNet
loop (implementations/matgl/models/tensornet.py:119-131 + the
Distributed.atom_transfer slice copies): each rank owns one slab
partition, runs the embedding and the interaction layers on it
(tensornet_ops, shared with tensornet.TensorNet_Dist), and exchanges the
flattened [n, 9C] border node tensors with its slab neighbors through the
HaloExchange autograd Function the CHGNet and MACE engines use
(distmlip_amd/runtime.py).

Divergences:
  * the halo AFTER the last layer is skipped — the reference performs it
    (tensornet.py:128 runs every iteration) but the readout only sums
    owned atoms, so nothing downstream of it reaches the energy; numerics
    are identical (the MACE engine's documented divergence);
  * one halo after the embedding, whose per-node sums a partition holds
    for its owned nodes only (tensornet.py module docstring);
  * per-rank geometry (no GPU0 serialization), forces assembled by one
    reverse halo-add of position gradients, one scalar all-reduce.
"""
from __future__ import annotations

import os as _os
from copy import deepcopy
from typing import Optional

import numpy as np
import torch
import torch.distributed as dist

from distmlip_amd import tensornet_ops as tno
from distmlip_amd.chgnet import PartitionData
from distmlip_amd.dist import Distributed
from distmlip_amd.ops_base import default_ops_factory
from distmlip_amd.runtime import HaloExchange, _HaloSeq, _exchange, halo_plan
from distmlip_amd.tensornet_model import TensorNetCore


class TensorNetSpmdEngine:
    """Per-rank TensorNet E+F(+stress) engine."""

    def __init__(self, core: TensorNetCore, world: int, threads: int = 8,
                 device: Optional[str] = None, ops=None,
                 gpu_build: str = "auto"):
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        assert world == 1 or dist.is_initialized()
        self.world = world
        self.config = core.config
        if self.config.is_intensive:
            raise NotImplementedError(
                "is_intensive = True is not supported by distributed "
                "inference")
        if device is None:
            device = f"cuda:{torch.cuda.current_device()}"
        self.device = torch.device(device)
        self.core = deepcopy(core).to(self.device).eval()
        self.core.requires_grad_(False)      # inference engine
        self.ops = ops if ops is not None else default_ops_factory(self.device)
        self.threads = threads
        if gpu_build not in ("auto", "fast", "off"):
            raise ValueError(f"gpu_build must be 'auto', 'fast' or 'off', "
                             f"got {gpu_build!r}")
        self.gpu_build = gpu_build
        self.float_th = self.core.linear.weight.dtype

    def build_graph(self, structure) -> Distributed:
        focus = self.rank if self.world > 1 else -1
        return Distributed.create_distributed(
            cart_coords=structure.cart_coords,
            frac_coords=structure.frac_coords,
            lattice_matrix=structure.lattice,
            num_partitions=self.world, pbc=structure.pbc,
            cutoff=self.config.cutoff, three_body_cutoff=0.0,
            use_bond_graph=False, num_threads=self.threads,
            focus_partition=focus)

    # -- one E+F step ------------------------------------------------------

    def step(self, structure, dist_info: Optional[Distributed] = None,
             calc_stresses: bool = False):
        r, P = self.rank, self.world
        cfg, core, ops, dev = self.config, self.core, self.ops, self.device
        ft = self.float_th
        C = cfg.units

        gpu_pd = None
        if dist_info is None:
            from distmlip_amd import gpu_graph
            if (dev.type == "cuda"
                    and not getattr(self.ops, "is_reference", False)
                    and _os.environ.get("DM_NO_GPU_BUILD") != "1"
                    and gpu_graph.engages(structure, cfg.cutoff,
                                          self.gpu_build)):
                if P == 1:
                    gpu_pd = gpu_graph.build(structure, cfg.cutoff, 0.0,
                                             1e-8, False, dev)
                else:
                    gpu_pd = gpu_graph.build_partition(
                        structure, P, r, cfg.cutoff, 0.0, 1e-8, False, dev)
            else:
                dist_info = self.build_graph(structure)
        if gpu_pd is not None and P == 1:
            pd = gpu_pd
            plan = []
            gids = np.arange(pd.n_atoms)
            n_owned = pd.n_atoms
        elif gpu_pd is not None:
            pd = gpu_pd
            plan = halo_plan(pd.markers, r, P)
            gids = pd.global_ids
            n_owned = pd.n_owned
        else:
            pd = PartitionData(dist_info, r, dev, use_bond_graph=False)
            plan = halo_plan(dist_info.markers[r], r, P)
            gids = np.asarray(dist_info.global_ids[r])
            n_owned = dist_info.num_owned_atoms(r)
        halo_seq = _HaloSeq()

        def halo(X):
            if not plan:
                return X
            flat = HaloExchange.apply(X.reshape(X.shape[0], 9 * C), plan,
                                      halo_seq)
            return flat.view(-1, 9, C)

        # ---- per-rank geometry
        lat0 = torch.tensor(np.asarray(structure.lattice), dtype=ft,
                            device=dev)
        strain = lat0.new_zeros(3, 3)
        if calc_stresses:
            strain.requires_grad_(True)
        lattice = lat0 @ (torch.eye(3, device=dev, dtype=ft) + strain)

        frac_src = np.asarray(structure.frac_coords)
        frac_local = torch.tensor(frac_src[gids], dtype=ft, device=dev)
        pos = frac_local @ lattice
        if not pos.requires_grad:
            pos.requires_grad_(True)
        pos.retain_grad()

        spec = np.asarray(structure.species)
        species = torch.tensor(spec[gids], dtype=torch.long, device=dev)

        if gpu_pd is not None:
            off_local = pd.off_i8.to(ft)
        elif (csr := dist_info.csr_parts[r]
              if getattr(dist_info, "csr_parts", None) else None) is not None:
            off_local = torch.from_numpy(csr["offsets_i8"]).to(dev).to(ft)
        else:
            egids = np.asarray(dist_info.L2G_DE_mapping_list[r])
            off_local = torch.tensor(np.asarray(dist_info.py_offsets)[egids],
                                     dtype=ft, device=dev)

        src_l, dst_l = pd.src.long(), pd.dst.long()
        vectors = pos[dst_l] + off_local @ lattice - pos[src_l]
        vhat, rbf, cut = tno.edge_basis(vectors, core)

        X = halo(tno.tn_embedding(core, species, vhat, rbf, cut, pd, ops))
        for i, layer in enumerate(core.layers):
            X = tno.tn_layer(layer, X, rbf, cut, pd, ops, cfg.group)
            if i < cfg.nblocks - 1:
                X = halo(X)          # atom_transfer (tensornet.py:128)

        es = tno.tn_node_energy(core, X[:n_owned])
        loss = core.data_std * es.sum()
        e_ref = core.element_refs[species[:n_owned]].sum()

        grads = [pos, strain] if calc_stresses else [pos]
        gv = torch.autograd.grad(loss, grads)
        pos_grad = gv[0]

        recvs = _exchange(pos_grad, plan, reverse=True)
        pos_grad = pos_grad.clone()
        for (q, ss, se, rs, re) in plan:
            if se > ss:
                pos_grad[ss:se] += recvs[q]
        forces_owned = -pos_grad[:n_owned]

        scal = torch.stack([loss.detach(), e_ref.detach()])
        if P > 1:
            dist.all_reduce(scal)
        total_e = scal[0] + scal[1] + core.data_mean.detach()

        out = {"energy": total_e, "forces_owned": forces_owned,
               "n_owned": n_owned,
               "global_ids_owned": gids[:n_owned]}
        if calc_stresses:
            sg = gv[1].detach().clone()
            if P > 1:
                dist.all_reduce(sg)
            volume = float(np.abs(np.linalg.det(
                np.asarray(structure.lattice))))
            out["stress"] = -sg / volume * -160.21766208
        return out
