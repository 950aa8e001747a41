"""A swarm in a mapped world: the closed loop of sensing (include/quasar_slam.h, "sensing a world"), mapping and target
assignment, so that the exploration strategies can be compared by what they uncover and not by the cost of one call.

`world` and `mapper` are two QuasarMapper contexts on one GPU.  The world is any context whose map is the truth (a maze painted
through update_rays, a restored checkpoint, a session's map); the mapper is what the swarm knows.  Each tick the world casts the
bots' sweeps or packets into a device buffer and the mapper ingests that buffer: the records never leave the GPU.  Only the
poses (12 bytes a bot) go up and the targets come down.

Device buffers are torch tensors, so torch is imported here -- before the HIP library is first loaded, as _lib.load() asks."""
import math

import numpy as np
import torch

from . import protocol as P
from .mapper import QuasarMapper

STRATEGIES = ("nearest", "by_path", "by_territory", "by_gain")
SIM_MIN_DIST_M = 0.02           # the sim mapper's trust filters start below one cell: a wall in the next cell returns d = res
SENSOR_ANGLES = (0.0, math.pi / 2, math.pi, -math.pi / 2)     # front, left, back, right (dual_bot_mapper.py:61-66)


def body_ranges(pose, agent, ranges, radius_m, max_range):
    """The four f32 ranges of each packet with the other bots' bodies in the way: float32 [n, 4].  pose float [n, 3] (x, y, yaw),
    agent [n], ranges float32 [n, 4] as the world returned them.  Every bot is a disc of radius_m about its pose; a beam takes
    the nearest intersection (ray-circle, fp64) with a disc of another agent when that is nearer than the world's return.  A
    beam without a return within max_range (not 0 < d <= max_range) takes the body distance when that lies within max_range."""
    pose = np.asarray(pose, dtype=np.float64).reshape(-1, 3)
    agent = np.asarray(agent).reshape(-1)
    out = np.array(ranges, dtype=np.float32).reshape(-1, 4)
    r2 = float(radius_m) ** 2
    for i in range(len(pose)):
        other = agent != agent[i]
        if not other.any():
            continue
        cx, cy = pose[other, 0] - pose[i, 0], pose[other, 1] - pose[i, 1]
        for s, ang in enumerate(SENSOR_ANGLES):
            a = pose[i, 2] + ang
            ux, uy = math.cos(a), math.sin(a)
            tca = cx * ux + cy * uy                              # along the beam to the point nearest the disc's centre
            off2 = cx * cx + cy * cy - tca * tca
            t = tca - np.sqrt(np.maximum(r2 - off2, 0.0))        # the near intersection
            t = t[(off2 <= r2) & (t > 0.0)]                      # (a disc behind the sensor, or around it, returns nothing)
            if not len(t):
                continue
            body = float(t.min())
            d = float(out[i, s])
            world = d if 0.0 < d <= max_range else math.inf
            if body < world and body <= max_range:
                out[i, s] = np.float32(body)
    return out


def body_sweep_ranges(pose, agent, ranges, radius_m, max_range):
    """body_ranges for sweeps: the 181 f32 ranges of each sweep with the other bots' bodies in the way, float32 [n, 181].  pose
    float [n, 3] (x, y, yaw), agent [n], ranges float32 [n, 181] as the world returned them; beam i points along
    yaw + radians(i - 90).  Every bot is a disc of radius_m about its pose; a beam takes the nearest intersection (ray-circle,
    fp64) with a disc of another agent when that is nearer than the world's return.  A beam without a return within max_range
    (not 0 < d <= max_range) takes the body distance when that lies within max_range."""
    pose = np.asarray(pose, dtype=np.float64).reshape(-1, 3)
    agent = np.asarray(agent).reshape(-1)
    out = np.array(ranges, dtype=np.float32).reshape(-1, P.SWEEP_BEAMS)
    r2 = float(radius_m) ** 2
    beam = np.array([math.radians(i - 90) for i in range(P.SWEEP_BEAMS)])
    for i in range(len(pose)):
        other = agent != agent[i]
        if not other.any():
            continue
        cx, cy = pose[other, 0] - pose[i, 0], pose[other, 1] - pose[i, 1]                # [m]
        a = pose[i, 2] + beam
        ux, uy = np.cos(a)[:, None], np.sin(a)[:, None]                                  # [181, 1]
        tca = cx[None, :] * ux + cy[None, :] * uy                # along each beam to the point nearest each disc's centre
        off2 = (cx * cx + cy * cy)[None, :] - tca * tca
        t = tca - np.sqrt(np.maximum(r2 - off2, 0.0))            # the near intersection
        t = np.where((off2 <= r2) & (t > 0.0), t, np.inf)        # (a disc behind the sensor, or around it, returns nothing)
        body = t.min(axis=1)
        d = out[i].astype(np.float64)
        world = np.where((0.0 < d) & (d <= max_range), d, np.inf)
        take = (body < world) & (body <= max_range)
        out[i, take] = body[take].astype(np.float32)
    return out


class SwarmSim:
    """n bots at world poses float32 [n, 3] (x, y, yaw); bot k has agent id k + 1, so the mapper needs max_agent >= n.

    kind       "sweeps" (751-byte records, 181 beams over the front half plane) or "packets" (42-byte records, four beams)
    max_range  the sensor's reach R in metres; speed  metres per second in drive()
    noise      noise_amp, dropout, seed of QuasarMapper.sense_params; record k of tick t draws as record t * n + k
    bodies     None, or the bots' body radius in metres (kind "packets" only): the bots see each other.  The tick then takes the
               host path: the world's packets come to the host, body_ranges shortens the beams that end on another bot, and the
               mapper ingests the host array"""

    def __init__(self, world, mapper, poses, kind="sweeps", max_range=P.MAX_DIST_M, speed=0.5, bodies=None, **noise):
        if kind not in ("sweeps", "packets"):
            raise ValueError("kind must be 'sweeps' or 'packets'")
        if bodies is not None and kind != "packets":
            raise ValueError("bodies needs kind='packets'")
        self.bodies = None if bodies is None else float(bodies)
        self._h_pkts = None
        unknown = set(noise) - {"noise_amp", "dropout", "seed"}
        if unknown:
            raise ValueError(f"unknown noise parameters: {sorted(unknown)}")
        if (world.size, world.res, world.ox, world.oy) != (mapper.size, mapper.res, mapper.ox, mapper.oy):
            raise ValueError("world and mapper must share one grid geometry")
        self.world, self.mapper, self.kind = world, mapper, kind
        self.max_range, self.speed, self.noise = float(max_range), float(speed), noise
        self.poses = np.array(poses, dtype=np.float32).reshape(-1, 3)
        self.n = len(self.poses)
        if not 1 <= self.n <= mapper.max_agent:
            raise ValueError("the mapper's max_agent must cover the bots")
        self.stride = P.PACKET_SIZE_V0_ODO if kind == "sweeps" else P.PACKET_SIZE
        self.truth = world.grid_i8()                       # the host copy drive() collides with
        dev = torch.device("cuda", int(world.cfg.device))
        self._d_pose = torch.zeros((self.n, 3), dtype=torch.float32, device=dev)
        self._d_agent = torch.arange(1, self.n + 1, dtype=torch.uint8, device=dev)
        self._d_enc = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self._d_pkts = torch.zeros(self.n * self.stride, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        self.tick = 0
        self.history = []                                  # known_cells() after each step

    @staticmethod
    def make_mapper(world, max_agent, max_range=P.MAX_DIST_M, **kw):
        """A mapper for a swarm in `world`: the same geometry, and trust filters (sweeps: set_sweep_filter, packets: min_dist /
        max_dist) whose lower bound lies below one cell.  With the defaults a wall in the neighbouring cell (d = res) is "too
        close" and the ingest rule casts a full-length free ray through it."""
        m = QuasarMapper(world.size, world.res, world.ox, world.oy, max_agent=max_agent, min_dist=SIM_MIN_DIST_M,
                         max_dist=float(max_range), device=int(world.cfg.device), **kw)
        m.set_sweep_filter(SIM_MIN_DIST_M, float(max_range))
        return m

    # -- sense: world -> device buffer -> mapper ------------------------------------------------------------------------------
    def sense(self):
        """Cast every bot's record from the world and ingest it into the mapper; the records stay on the device.  Ordering
        between the two contexts' streams is by qs_sync: on the mapper before the buffer is overwritten (its last ingest has
        read it), on the world before the mapper is handed the buffer (the cast has written it)."""
        if self.bodies is not None:
            kw = dict(max_range=self.max_range, first_record=self.tick * self.n, **self.noise)
            agent = np.arange(1, self.n + 1, dtype=np.uint8)
            pk = self.world.sense_packets(self.poses, agent, enc=np.full(self.n, self.tick, dtype=np.int32), **kw)
            rec = pk.view(P.PACKET_DTYPE).reshape(-1)
            d4 = np.stack([rec[k] for k in ("front", "left", "back", "right")], axis=1)
            d4 = body_ranges(self.poses, agent, d4, self.bodies, self.max_range)
            for j, k in enumerate(("front", "left", "back", "right")):
                rec[k] = d4[:, j]
            self._h_pkts = pk
            self.mapper.ingest_array(pk)
            return
        self.mapper.sync()
        self._d_pose.copy_(torch.from_numpy(self.poses))   # a blocking copy: complete when it returns
        self._d_enc.fill_(self.tick)
        torch.cuda.synchronize(self._d_pose.device)
        kw = dict(max_range=self.max_range, first_record=self.tick * self.n, **self.noise)
        if self.kind == "sweeps":
            self.world.sense_sweeps_device(self._d_pose, self._d_agent, self.n, self._d_pkts, self.stride, d_enc=self._d_enc, **kw)
        else:
            self.world.sense_packets_device(self._d_pose, self._d_agent, self.n, self._d_pkts, d_enc=self._d_enc, **kw)
        self.world.sync()
        if self.kind == "sweeps":
            self.mapper.ingest_sweeps_device(self._d_pkts.data_ptr(), self.n, self.stride)
        else:
            self.mapper.ingest_device(self._d_pkts.data_ptr(), self.n, self.stride)

    def last_records(self):
        """uint8 [n, stride]: the records of the last sense() (a copy to the host, for inspection)."""
        self.mapper.sync()
        if self._h_pkts is not None:
            return self._h_pkts.copy()
        return self._d_pkts.cpu().numpy().reshape(self.n, self.stride)

    # -- drive: host only, deterministic ----------------------------------------------------------------------------------------
    def _blocked(self, x, y):
        gx, gy = int((x - self.world.ox) / self.world.res), int((y - self.world.oy) / self.world.res)     # world_to_grid
        size = self.world.size
        return 0 <= gx < size and 0 <= gy < size and self.truth[gy, gx] == P.CELL_OCCUPIED

    def drive(self, waypoints, dt=1.0):
        """Move each bot toward its waypoint (float [n, 2]; NaN = none) by at most speed * dt, in steps of a quarter cell,
        stopping before a cell that is OCCUPIED in the world; its yaw becomes the heading.  A bot without a waypoint, or within
        half a cell of it, stays and turns a quarter left, so that a sweep's front half plane comes round."""
        wp = np.asarray(waypoints, dtype=np.float64).reshape(self.n, 2)
        sub = self.world.res / 4
        for k in range(self.n):
            x, y, yaw = (float(v) for v in self.poses[k])
            dx, dy = wp[k, 0] - x, wp[k, 1] - y
            dist = math.hypot(dx, dy)                      # (NaN without a waypoint)
            if not dist >= self.world.res / 2:
                self.poses[k, 2] = np.float32(math.atan2(math.sin(yaw + math.pi / 2), math.cos(yaw + math.pi / 2)))
                continue
            ux, uy = dx / dist, dy / dist
            left = min(self.speed * dt, dist)
            while left > 0.0:
                s = min(sub, left)
                nx, ny = x + s * ux, y + s * uy
                if self._blocked(nx, ny):
                    break
                x, y, left = nx, ny, left - s
            self.poses[k] = (x, y, math.atan2(dy, dx))

    # -- targets ------------------------------------------------------------------------------------------------------------------
    def targets(self, strategy, **kw):
        """float64 [n, 2]: where each bot should head next by one of STRATEGIES (NaN = nothing assigned): the centroid itself for
        "nearest" (the reference's greedy rule, no planner), else the waypoint of the bot's path to its target."""
        xy = self.poses[:, :2].astype(np.float64)
        if strategy == "nearest":
            return self.mapper.frontier_targets(xy, **kw)[1]
        if strategy == "by_path":
            return self.mapper.frontier_targets_by_path(xy, **kw)["waypoint"]
        if strategy == "by_territory":
            return self.mapper.frontier_targets_by_territory(xy, **kw)["waypoint"]
        if strategy == "by_gain":
            return self.mapper.frontier_targets_by_gain(xy, **kw)["waypoint"]
        raise ValueError(f"strategy must be one of {STRATEGIES}")

    def step(self, strategy="by_path", dt=1.0, **kw):
        """One tick: sense, assign targets, drive.  Returns known_cells() (also appended to history)."""
        self.sense()
        self.drive(self.targets(strategy, **kw), dt)
        self.tick += 1
        known = self.known_cells()
        self.history.append(known)
        return known

    def known_cells(self):
        """Cells of the mapper with a nonzero stamp (FREE or OCCUPIED)."""
        return int(np.count_nonzero(self.mapper.grid_i8() != P.CELL_UNKNOWN))
