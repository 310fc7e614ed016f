"""DM_MACE_CONV=radial where the kernels cannot run (CPU, reference ops):
the engine behaves as if the variable were unset."""
import numpy as np
import torch

from distmlip_amd.mace_model import MACEConfig, MACECore
from distmlip_amd.mace_runtime import MaceSpmdEngine
from distmlip_amd.structures import diamond_si
from oracle.chgnet_ref import CpuRefOps


def test_radial_falls_back_on_cpu(monkeypatch):
    s = diamond_si((3, 2, 2), jitter=0.1, seed=2)
    s.species = np.asarray(s.species) % 3
    core = MACECore.seeded(MACEConfig(n_elements=3, channels=16),
                           seed=9).double()
    eng = MaceSpmdEngine(core, world=1, threads=2, device="cpu",
                         ops=CpuRefOps())
    monkeypatch.delenv("DM_MACE_CONV", raising=False)
    ref = eng.step(s)
    monkeypatch.setenv("DM_MACE_CONV", "radial")
    out = eng.step(s)
    assert out["energy"].item() == ref["energy"].item()
    assert torch.equal(out["forces_owned"], ref["forces_owned"])
