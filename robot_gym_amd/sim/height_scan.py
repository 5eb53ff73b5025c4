"""Terrain height scan: an elevation sensor for the robots of BatchedSRBSim (include/rg_scan.h).

A fixed nx x ny grid of points in the robot's yaw frame (x forward, y left); under each point the height of the body above
the ground, less the nominal body height, clipped and scaled: float32 [nx * ny, B], component-major like every observation
the policy kernels read.  It is a height sample, not a ray -- nothing occludes -- and roll and pitch do not tilt the grid.  It
is exact: noise, dropout and latency are SensorModel's (robot_gym_amd/sim/sensor_model.py).  The ground is the simulator's own;
all arithmetic happens in librg_mpc.so.

    sim = BatchedSRBSim(B, cfg, terrain=RandomTerrain())
    scan = HeightScan()                  # 8 x 6 points, 0.1 m apart, from 0.2 m behind the body to 0.5 m ahead
    scan.bind(sim)
    heights = scan.observe(sim.state)    # [48, B]

BatchedGoEnv(..., height_scan=HeightScan()) binds it and appends the scan to its observation.
"""
import numpy as np
import torch

from robot_gym_amd.core import scan_abi, srb_abi


class HeightScan:
    """The fields of rg_scan_config (defaults: scan_abi.DEFAULTS; z_offset None: the body_height of the simulator's config;
    clip 0: no clipping).  The library checks them at bind(); nothing touches the device before it."""

    def __init__(self, nx=8, ny=6, x_first=-0.2, dx=0.1, y_first=-0.25, dy=0.1, z_offset=None, clip=1.0, scale=1.0):
        self.settings = dict(nx=int(nx), ny=int(ny), x_first=float(x_first), dx=float(dx), y_first=float(y_first), dy=float(dy),
                             z_offset=None if z_offset is None else float(z_offset), clip=float(clip), scale=float(scale))
        self.nx, self.ny = self.settings["nx"], self.settings["ny"]
        self.num_points = self.nx * self.ny
        self.z_offset, self.clip, self.scale = self.settings["z_offset"], self.settings["clip"], self.settings["scale"]
        self.batch = self.device = self.terrain = self._handle = None

    @property
    def points(self):
        """float64 [nx * ny, 2]: the points' (x, y) in the yaw frame, point k = a * ny + c at grid node (a, c)."""
        s = self.settings
        a, c = np.meshgrid(np.arange(self.nx, dtype=np.float64), np.arange(self.ny, dtype=np.float64), indexing="ij")
        return np.stack([s["x_first"] + a.ravel() * s["dx"], s["y_first"] + c.ravel() * s["dy"]], axis=1)

    def bind(self, sim):
        """Creates the handle for the simulator's batch and device (z_offset None: its config's body_height) and takes the
        terrain the simulator has bound.  Returns self."""
        if self._handle is not None:
            raise RuntimeError("HeightScan: already bound (one scanner per simulator)")
        self.batch, self.device = sim.batch, sim.device
        self._handle = scan_abi.ScanHandle(sim.batch, sim.cfg, sim.device, **self.settings)
        self.z_offset = float(self._handle.fields["z_offset"])
        self.set_terrain(sim.terrain)
        return self

    def set_terrain(self, terrain):
        """The ground to scan: the RandomTerrain / GridTerrain a simulator has bound (after sim.set_terrain(terrain)), an
        srb_abi.CTerrain of the caller's own tensors, or None for the plane.  A terrain object is NOT bound again: the scanner
        reads the key / heights tensors the simulator reads, so a cloned robot's scan sees its source's ground."""
        if self._handle is None:
            raise RuntimeError("HeightScan: bind(sim) first")
        self._handle.set_terrain(terrain if terrain is None or isinstance(terrain, srb_abi.CTerrain) else terrain.descriptor())
        self.terrain = terrain   # keeps the terrain's tensors alive

    def _rows(self, t, name):
        N, B = self.num_points, self.batch
        ok = (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == self.device and tuple(t.shape) == (N, B)
              and (t.stride() == (B, 1) or B == 1 and t.stride(0) == 1))
        if not ok:
            raise ValueError(f"observe: {name} must be a float32 [{N},{B}] tensor on {self.device} with row stride {B} "
                             "(a whole tensor, or rows of a taller [*, B] one)")
        return t.data_ptr()

    def observe(self, state, out=None, mask=None, prev=None):
        """The scan of the simulator state `state` (float64 [43, B]) into out, float32 [nx * ny, B] (None: a new tensor); out and
        prev may be row views of a taller [*, B] buffer.  mask: int32 [B] device tensor, None: all robots.  For a masked
        robot, prev (if given) first takes out's old column, then out is written; any other robot is touched in neither.
        Enqueued on the current stream; nothing waits.  Returns out."""
        if self._handle is None:
            raise RuntimeError("HeightScan: bind(sim) first")
        B = self.batch
        if not torch.is_tensor(state) or state.dtype != torch.float64 or tuple(state.shape) != (srb_abi.STATE_ROWS, B) or not state.is_contiguous() or state.device != self.device:
            raise ValueError(f"observe: state must be a contiguous float64 [{srb_abi.STATE_ROWS},{B}] tensor on {self.device}")
        if out is None:
            out = torch.zeros(self.num_points, B, dtype=torch.float32, device=self.device)
        mp = None
        if mask is not None:
            if not torch.is_tensor(mask) or mask.dtype != torch.int32 or tuple(mask.shape) != (B,) or not mask.is_contiguous() or mask.device != self.device:
                raise ValueError(f"observe: mask must be a contiguous int32 [{B}] tensor on {self.device}")
            mp = mask.data_ptr()
        self._handle.observe(state.data_ptr(), mp, self._rows(out, "out"), None if prev is None else self._rows(prev, "prev"))
        return out

    def close(self):
        if self._handle is not None:
            self._handle.close()
