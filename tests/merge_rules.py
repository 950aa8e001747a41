"""The rules of the map merge session (include/quasar_slam.h: "map merge session"; server_nodes/map_merger.py:35-62) restated
in numpy, for the CPU and the GPU tests: the callback's flow, rule 5's transform with every product and sum written out
(no `@`: a BLAS may fuse or reorder), and the maps both tests feed.  Registration, down-sampling, grid_to_pcd and
rasterise are whatever functions the caller hands in (the CPU test: the oracle's; the GPU test: the mapper's host-to-host
entry points), as match_rules.py takes the device's rotations."""
import numpy as np

EMPTY, ADOPTED, MERGED, REJECTED = "empty", "adopted", "merged", "rejected"
RES, OX, OY = 0.05, -12.8, -12.8           # geometry of tests/golden/session_512.npz


def moved(local, T):
    """Rule 5: x' = (T[0]*x + T[1]*y) + T[2], y' = (T[3]*x + T[4]*y) + T[5], each operation rounded on its own."""
    T = np.asarray(T, dtype=np.float64).reshape(3, 3)
    x, y = local[:, 0], local[:, 1]
    out = np.empty_like(local)
    out[:, 0] = (T[0, 0] * x + T[0, 1] * y) + T[0, 2]
    out[:, 1] = (T[1, 0] * x + T[1, 1] * y) + T[1, 2]
    return out


class Session:
    """MapMerger's state and map_callback over pluggable steps:
    grid_to_pcd(grid, res, ox, oy) -> [n, 2]; register(local, cloud, threshold, iterations) -> (T, fitness, rmse, iterations);
    voxel(xy, res) -> [m, 2]; rasterise(xy, res) -> (grid, origin)."""

    def __init__(self, grid_to_pcd, register, voxel, rasterise, icp_threshold=1.0, icp_iterations=30, min_fitness=0.6):
        self.grid_to_pcd, self.register, self.voxel, self.rasterise = grid_to_pcd, register, voxel, rasterise
        self.icp_threshold, self.icp_iterations, self.min_fitness = icp_threshold, icp_iterations, min_fitness
        self.cloud = np.zeros((0, 2))
        self.res, self.origin = 0.05, [0.0, 0.0]

    def callback(self, grid, res, ox, oy):
        """-> dict like QuasarMapper.merge_grid's."""
        local = self.grid_to_pcd(grid, res, ox, oy)
        r = {"status": EMPTY, "T": np.eye(3), "fitness": 0.0, "rmse": 0.0, "iterations": 0, "n_local": len(local)}
        if len(local) == 0:                                               # :37-38
            pass
        elif len(self.cloud) == 0:                                        # :40-43
            self.cloud, self.res, self.origin = local, res, [ox, oy]
            r["status"] = ADOPTED
        else:
            T, fit, rm, it = self.register(local, self.cloud, self.icp_threshold, self.icp_iterations)   # :45-52
            r.update(T=np.asarray(T).reshape(3, 3), fitness=fit, rmse=rm, iterations=it)
            if fit < self.min_fitness:                                    # :54-56
                r["status"] = REJECTED
            else:                                                         # :58-60
                self.cloud = self.voxel(np.concatenate([self.cloud, moved(local, T)]), self.res)
                r["status"] = MERGED
        r["n_global"] = len(self.cloud)
        return r

    def publish(self):
        return self.rasterise(self.cloud, self.res) if len(self.cloud) else (None, None)


# ---- the maps of the tests ----------------------------------------------------------------------------------------------
def occupied_points(grid, res=RES, ox=OX, oy=OY):
    rows, cols = np.nonzero(grid > 50)                                    # row-major, as np.argwhere
    return np.stack([cols * res + ox, rows * res + oy], axis=1)


def rotated_map(grid, degrees, res=RES, ox=OX, oy=OY):
    """The room as an agent whose frame is turned by `degrees` about the middle of the occupied cells' box reports it: the
    occupied cells' centres rotated and rasterised again (nearest cell) on a grid of the same geometry; everything else
    unknown."""
    p = occupied_points(grid, res, ox, oy)
    c = 0.5 * (p.min(0) + p.max(0))
    a = np.radians(degrees)
    q = np.empty_like(p)
    q[:, 0] = np.cos(a) * (p[:, 0] - c[0]) - np.sin(a) * (p[:, 1] - c[1]) + c[0]
    q[:, 1] = np.sin(a) * (p[:, 0] - c[0]) + np.cos(a) * (p[:, 1] - c[1]) + c[1]
    col = np.floor((q[:, 0] - ox) / res + 0.5).astype(np.int64)
    row = np.floor((q[:, 1] - oy) / res + 0.5).astype(np.int64)
    out = np.full(grid.shape, -1, dtype=np.int8)
    out[row, col] = 100
    return out


def with_corner_block(grid, edge):
    """The map plus an edge x edge occupied block in the grid's corner (more than 1 m from every cell of the room: its cells
    never find a correspondence, so the fitness of the map against itself is occupied / (occupied + edge^2))."""
    out = grid.copy()
    out[:edge, :edge] = 100
    return out


def sequence(grid):
    """The six-map sequence: (name, grid, res, ox, oy, status the callback must report)."""
    low = np.where(np.arange(grid.shape[0])[:, None] < 270, grid, np.int8(-1)).astype(np.int8)
    far = np.full((64, 64), -1, dtype=np.int8)
    far[10:20, 10:20] = 100
    return [("first", grid, RES, OX, OY, ADOPTED),
            ("shifted", grid, RES, OX + 0.10, OY - 0.15, MERGED),
            ("rot3", rotated_map(grid, 3.0), RES, OX, OY, MERGED),
            ("rot12", rotated_map(grid, 12.0), RES, OX, OY, MERGED),
            ("rows_below_270", low, RES, OX, OY, MERGED),
            ("far", far, RES, 300.0, 300.0, REJECTED)]


def gate_cases(grid):
    """(name, grid, exact fitness against the map itself, status): count ratios on either side of min_fitness = 0.6."""
    n = int((grid > 50).sum())
    return [("block10", with_corner_block(grid, 10), n / (n + 100), MERGED),
            ("block20", with_corner_block(grid, 20), n / (n + 400), REJECTED)]
