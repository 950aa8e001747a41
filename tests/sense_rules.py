"""CPU restatement of the sensing rules S1-S8 of include/quasar_slam.h ("sensing a world"), for the tests.

Grids are OccupancyGrid.grid arrays (int8 [size, size] indexed [gy, gx]: -1 UNKNOWN, 0 FREE, 100 OCCUPIED), which is the stamp
reading of the device (odd stamp = OCCUPIED).  Trigonometry is Python's math.cos / math.sin (glibc); the device's may differ
in the last bit, which can move a far cell only when the far point lies on a cell boundary: edge_beams() lists those beams."""
import math

import numpy as np

import plan_rules as R

CLAMP = 1 << 30                 # cells beyond +-2^30 are clamped there (raycast_common.h); every grid is < 2^14 wide
MAX_CELLS = 255                 # QS_SENSE_MAX_CELLS
BEAMS = 181
PACKET_ANGLES = (0.0, math.pi / 2, math.pi, -math.pi / 2)       # front, left, back, right
MASK = (1 << 64) - 1
EDGE_BAND = 1e-6


def cell(w, o, res):
    """S2: world_to_grid, clamped; None where CPython's int() would raise or the cell is beyond 9e15."""
    q = (w - o) / res
    if not abs(q) < 9.0e15:
        return None
    return max(-CLAMP, min(CLAMP, int(q)))


def angles(yaw, beams):
    """S3: the beams' headings from the float32 yaw."""
    y = float(yaw)
    if beams == 4:
        return [y + a for a in PACKET_ANGLES]
    assert beams == BEAMS
    return [y + (i - 90) * (math.pi / 180) for i in range(BEAMS)]


def far_point(rx, ry, a, rng):
    """S4."""
    return rx + rng * math.cos(a), ry + rng * math.sin(a)


def draw(seed, record, beam):
    """S7: (u, z) of beam `beam` of record `record` (first_record + its index within the call)."""
    z = (seed + 0x9E3779B97F4A7C15 * (1 + record * 256 + beam)) & MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return (z >> 40) + ((z >> 16) & 0xFFFFFF), z


def noisy(d, noise_amp, dropout_q16, seed, record, beam):
    """S7: (d', dropped)."""
    if noise_amp == 0 and dropout_q16 == 0:
        return d, False
    u, z = draw(seed, record, beam)
    return d + noise_amp * (float(u) * 2.0 ** -24 - 1.0), (z & 0xFFFF) < dropout_q16


def walk(occ, start, far):
    """S5: the first OCCUPIED cell of _bresenham(start, far) after cell 0, or None.  occ: bool [size, size]."""
    h, w = occ.shape
    for x, y in R.bresenham(start[0], start[1], far[0], far[1])[1:]:
        if 0 <= x < w and 0 <= y < h and occ[y, x]:
            return x, y
    return None


def check_params(res, max_range, noise_amp=0.0, dropout_q16=0):
    """S8 (the part that is not about pointers): True when the call is valid."""
    if not (math.isfinite(max_range) and max_range > 0 and math.ceil(max_range / res) + 1 <= MAX_CELLS):
        return False
    return math.isfinite(noise_amp) and noise_amp >= 0 and 0 <= dropout_q16 <= 65536


def sense_ranges(grid, res, ox, oy, poses, beams=BEAMS, max_range=1.2, noise_amp=0.0, dropout_q16=0, seed=0, first_record=0,
                 no_return=0.0, records=None):
    """(ranges float32 [n, beams], hit_cell int32 [n, beams]) of float32 poses [n, 3].  records: restate only these record
    indices (the others' rows are left at no_return / -1)."""
    assert check_params(res, max_range, noise_amp, dropout_q16)
    occ = np.asarray(grid) == 100
    size = occ.shape[0]
    poses = np.asarray(poses, dtype=np.float32).reshape(-1, 3)
    n = len(poses)
    ranges = np.full((n, beams), no_return, dtype=np.float32)
    cells = np.full((n, beams), -1, dtype=np.int32)
    for k in (range(n) if records is None else records):
        x, y, yaw = (float(v) for v in poses[k])
        if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(yaw)):
            continue
        x0, y0 = cell(x, ox, res), cell(y, oy, res)
        if x0 is None or y0 is None:
            continue
        for i, a in enumerate(angles(poses[k, 2], beams)):
            fx, fy = far_point(x, y, a, max_range)
            x1, y1 = cell(fx, ox, res), cell(fy, oy, res)
            if x1 is None or y1 is None:
                continue
            hit = walk(occ, (x0, y0), (x1, y1))
            if hit is None:
                continue
            dx, dy = hit[0] - x0, hit[1] - y0
            d = res * math.sqrt(float(dx * dx + dy * dy))                      # S6
            d, dropped = noisy(d, noise_amp, dropout_q16, seed, first_record + k, i)
            f = np.float32(d)
            if not dropped and float(f) <= max_range:
                ranges[k, i] = f
                cells[k, i] = hit[1] * size + hit[0]
    return ranges, cells


def edge_beams(res, ox, oy, poses, beams=BEAMS, max_range=1.2, band=EDGE_BAND):
    """bool [n, beams]: the beams whose far-point quotient (w - o) / res lies within `band` of an integer on either axis.  The
    device is not compared on those."""
    poses = np.asarray(poses, dtype=np.float32).reshape(-1, 3)
    out = np.zeros((len(poses), beams), dtype=bool)
    for k, p in enumerate(poses):
        x, y, yaw = (float(v) for v in p)
        if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(yaw)):
            continue
        for i, a in enumerate(angles(p[2], beams)):
            fx, fy = far_point(x, y, a, max_range)
            for q in ((fx - ox) / res, (fy - oy) / res):
                if abs(q) < 9.0e15 and abs(q - round(q)) < band:      # (beyond 9e15 there is no cell and no return: S2)
                    out[k, i] = True
    return out


def zeros(v, n, dtype):
    return np.zeros(n, dtype=dtype) if v is None else np.broadcast_to(np.asarray(v, dtype=dtype), (n,))


def sense_sweeps(P, grid, res, ox, oy, poses, agent, enc=None, v2v=None, odometry=True, **kw):
    """uint8 [n, 751 | 743] through protocol.pack_sweeps."""
    poses = np.asarray(poses, dtype=np.float32).reshape(-1, 3)
    n = len(poses)
    ranges, _ = sense_ranges(grid, res, ox, oy, poses, BEAMS, **kw)
    return P.pack_sweeps(zeros(agent, n, np.uint8), poses[:, 0], poses[:, 1], poses[:, 2], ranges, enc=zeros(enc, n, np.int32),
                         v2v=zeros(v2v, n, np.uint32), odometry=odometry)


def sense_packets(P, grid, res, ox, oy, poses, agent, enc=None, v2v=None, landmark=None, **kw):
    """uint8 [n, 42] through protocol.pack_packets."""
    poses = np.asarray(poses, dtype=np.float32).reshape(-1, 3)
    n = len(poses)
    ranges, _ = sense_ranges(grid, res, ox, oy, poses, 4, **kw)
    return P.pack_packets(zeros(agent, n, np.uint8), poses[:, 0], poses[:, 1], poses[:, 2], zeros(enc, n, np.int32),
                          zeros(v2v, n, np.uint32), ranges, zeros(landmark, n, np.uint8))


def ranges_of(P, pkts):
    """float32 [n, 181 | 4]: the range fields of emitted records."""
    pkts = np.ascontiguousarray(pkts)
    if pkts.shape[1] == P.PACKET_SIZE:
        r = pkts.view(P.PACKET_DTYPE).reshape(-1)
        return np.stack([r["front"], r["left"], r["back"], r["right"]], axis=1)
    dt = P.PACKET_DTYPE_V0 if pkts.shape[1] == P.PACKET_SIZE_V0 else P.PACKET_DTYPE_V0_ODO
    return pkts.view(dt).reshape(-1)["ranges"].copy()


def chebyshev_to_occupied(occ_a, occ_b):
    """The largest Chebyshev distance from an OCCUPIED cell of a to the nearest OCCUPIED cell of b (0 when a has none)."""
    from scipy import ndimage
    if not occ_a.any():
        return 0
    if not occ_b.any():
        return max(occ_a.shape)
    d = ndimage.distance_transform_cdt(~occ_b, metric="chessboard")
    return int(d[occ_a].max())
