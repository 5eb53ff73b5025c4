"""The ground of the batched single-rigid-body simulator (include/rg_srb.h, "Terrain"): what BatchedSRBSim(..., terrain=)
and BatchedGoEnv(..., terrain=) take.  A terrain object describes the ground and holds its device tensors once a simulator
has bound it; the heights are computed in librg_mpc.so, never here.

    sim = BatchedSRBSim(B, cfg, terrain=RandomTerrain())            # the reference's `random` world, one per robot
    sim = BatchedSRBSim(B, cfg, terrain=GridTerrain(heights, 0.05)) # a heightfield of your own, shared by all robots
"""
import numpy as np
import torch

from robot_gym_amd.core import srb_abi


class RandomTerrain:
    """The reference's `random` heightfield (model/world/terrain.py), stateless and unbounded: vertices every `cell` metres,
    heights uniform in [0, amplitude) and constant over 2 x 2 vertex groups, a pure function of (seed, key, vertex).  keys:
    int64 [B] values, the world each robot walks in (equal keys: the same world); None: arange(B), one world per robot as
    the reference has one per env process.  `keys` is the device tensor after bind(); BatchedSRBSim.copy_columns copies it
    with the state, so a cloned robot walks on its source's ground."""

    def __init__(self, amplitude=0.06, cell=0.05, seed=0, keys=None):
        self.amplitude, self.cell, self.seed = float(amplitude), float(cell), int(seed)
        self._keys_arg = keys
        self.keys = None

    def bind(self, batch, device):
        k = self._keys_arg
        if k is None:
            self.keys = torch.arange(batch, dtype=torch.int64, device=device)
        else:
            k = k.to("cpu", torch.int64) if torch.is_tensor(k) else torch.as_tensor(np.asarray(k, dtype=np.int64))
            if tuple(k.shape) != (batch,):
                raise ValueError(f"RandomTerrain: keys must be [{batch}], got {list(k.shape)}")
            self.keys = k.to(device).contiguous()
        return self.descriptor()

    def descriptor(self):
        """The srb_abi.CTerrain of the bound terrain: it names the `keys` tensor bind() made, so whoever takes it (the simulator,
        a HeightScan) reads the same worlds."""
        if self.keys is None:
            raise RuntimeError("RandomTerrain: not bound yet (a simulator's set_terrain binds it)")
        return srb_abi.make_cterrain(srb_abi.TERRAIN_RANDOM, cell=self.cell, amplitude=self.amplitude, seed=self.seed, key=self.keys.data_ptr())


class GridTerrain:
    """heights [rows, cols] float64 vertex heights, heights[i, j] at (origin[0] + i cell, origin[1] + j cell), shared by all
    robots; beyond its edges the ground goes on at the border value.  `heights` is the device tensor after bind()."""

    def __init__(self, heights, cell, origin=(0.0, 0.0)):
        h = heights.detach().to("cpu", torch.float64) if torch.is_tensor(heights) else torch.as_tensor(np.asarray(heights, dtype=np.float64))
        if h.dim() != 2:
            raise ValueError(f"GridTerrain: heights must be [rows, cols], got {list(h.shape)}")
        if not bool(torch.isfinite(h).all()):
            raise ValueError("GridTerrain: heights must be finite")
        self._heights_host = h.contiguous()
        self.cell, self.origin = float(cell), (float(origin[0]), float(origin[1]))
        self.heights = None
        self.keys = None

    def bind(self, batch, device):
        self.heights = self._heights_host.to(device).contiguous()
        return self.descriptor()

    def descriptor(self):
        """The srb_abi.CTerrain of the bound terrain: it names the `heights` tensor bind() made."""
        if self.heights is None:
            raise RuntimeError("GridTerrain: not bound yet (a simulator's set_terrain binds it)")
        rows, cols = self.heights.shape
        return srb_abi.make_cterrain(srb_abi.TERRAIN_GRID, cell=self.cell, heights=self.heights.data_ptr(), rows=rows, cols=cols,
                                     x0=self.origin[0], y0=self.origin[1])
