"""The sensing rules S1-S8 (include/quasar_slam.h, "sensing a world") in their CPU restatement, tests/sense_rules.py: what the
GPU tests compare the device against, checked here on cases small enough to read, and once round the reference's update_ray."""
import importlib
import math

import numpy as np
import pytest

import plan_rules
import sense_rules as S
from conftest import load_pkg
from oracle import oracle as orc

RES, OX, OY, SIZE = 0.05, -5.0, -5.0, 200
# the largest Chebyshev distance between a sensed hit cell and the cell the reference's update_ray marks when it is fed the sensed
# range from the same pose along the same beam (test_round_trip_through_update_ray measures it; DESIGN.md 4.18 quotes it)
ROUND_TRIP_CELLS = 1


@pytest.fixture(scope="module")
def P():
    return importlib.import_module(load_pkg().__name__ + ".protocol")


def centre(gx, gy, yaw=0.0):
    return [OX + (gx + 0.5) * RES, OY + (gy + 0.5) * RES, yaw]


def empty():
    return np.zeros((SIZE, SIZE), dtype=np.int8)


def test_empty_world_returns_only_no_returns():
    poses = [centre(100, 100), centre(0, 0, 1.0), centre(199, 199, -2.0), [-9.0, 3.0, 0.3]]
    for beams in (181, 4):
        r, c = S.sense_ranges(empty(), RES, OX, OY, poses, beams, no_return=-1.0)
        assert (r == -1.0).all() and (c == -1).all()
    unknown = np.full((SIZE, SIZE), -1, dtype=np.int8)
    r, c = S.sense_ranges(unknown, RES, OX, OY, poses)
    assert (r == 0.0).all() and (c == -1).all()          # UNKNOWN does not block; the default no_return is 0.0f


@pytest.mark.parametrize("k", [1, 2, 7, 23])
def test_wall_straight_ahead(k):
    g = empty()
    g[:, 100 + k] = 100
    r, c = S.sense_ranges(g, RES, OX, OY, [centre(100, 60)], 4)
    assert r[0, 0] == np.float32(RES * k) and c[0, 0] == 60 * SIZE + 100 + k
    assert (r[0, 1:] == 0).all() and (c[0, 1:] == -1).all()
    r, c = S.sense_ranges(g, RES, OX, OY, [centre(100, 60)])
    assert r[0, 90] == np.float32(RES * k) and c[0, 90] == 60 * SIZE + 100 + k
    assert r[0, 0] == 0 and r[0, 180] == 0                # beams along the wall's direction never reach it


def test_occupied_start_cell_does_not_block():
    g = empty()
    g[60, 100] = 100
    g[60, 105] = 100
    r, c = S.sense_ranges(g, RES, OX, OY, [centre(100, 60)], 4)
    assert r[0, 0] == np.float32(RES * 5) and c[0, 0] == 60 * SIZE + 105
    assert (c[0, 1:] == -1).all()


def test_cells_outside_the_grid_are_skipped_not_stopped():
    g = empty()
    g[:, 3] = 100
    pose = centre(-10, 50)                                 # left of the grid, looking in
    assert S.cell(float(np.float32(pose[0])), OX, RES) == -9          # world_to_grid truncates toward zero: -9.5 -> -9
    r, c = S.sense_ranges(g, RES, OX, OY, [pose], 4)
    assert c[0, 0] == 50 * SIZE + 3 and r[0, 0] == np.float32(RES * 12)
    # from the inside looking out: the line leaves the grid and nothing stops it
    r, c = S.sense_ranges(g, RES, OX, OY, [centre(1, 50, math.pi)], 4)
    assert c[0, 0] == -1 and c[0, 2] == 50 * SIZE + 3


def test_a_hit_beyond_the_range_is_dropped():
    g = empty()
    g[:, 124] = 100
    # from 0.9 of the way through cell 100 the far point of a 1.2 m beam lies in cell 124, so the walk reaches the wall;
    # centre to centre that is 24 cells = f32(1.2) = 1.2000000476837158 > 1.2: no return
    pose = [OX + 100.9 * RES, OY + 60.5 * RES, 0.0]
    assert S.cell(S.far_point(float(np.float32(pose[0])), 0.0, 0.0, 1.2)[0], OX, RES) == 124
    r, c = S.sense_ranges(g, RES, OX, OY, [pose], 4, max_range=1.2, no_return=7.0)
    assert r[0, 0] == 7.0 and c[0, 0] == -1
    r, c = S.sense_ranges(g, RES, OX, OY, [pose], 4, max_range=1.25)
    assert r[0, 0] == np.float32(RES * 24) and c[0, 0] == 60 * SIZE + 124


def test_the_walk_goes_from_the_pose_outward():
    """_bresenham((0, 0), (2, 1)) passes (1, 0); _bresenham((2, 1), (0, 0)) passes (1, 1) instead."""
    fwd = plan_rules.bresenham(0, 0, 2, 1)
    back = plan_rules.bresenham(2, 1, 0, 0)
    assert fwd == [(0, 0), (1, 0), (2, 1)] and back == [(2, 1), (1, 1), (0, 0)]
    yaw, rng = math.atan2(1, 2), RES * math.hypot(2, 1)    # the far point is the centre of cell (+2, +1)
    for blocker, hit in (((1, 0), True), ((1, 1), False)):
        g = empty()
        g[80 + blocker[1], 80 + blocker[0]] = 100
        r, c = S.sense_ranges(g, RES, OX, OY, [centre(80, 80, yaw)], 4, max_range=rng + 1e-9)
        assert (c[0, 0] == (80 + blocker[1]) * SIZE + 80 + blocker[0]) == hit, (blocker, c[0])
        assert S.walk(g == 100, (80, 80), (82, 81)) == ((80 + blocker[0], 80 + blocker[1]) if hit else None)


def _room(seed=7, size=256):
    rng = np.random.default_rng(seed)
    g = np.zeros((size, size), np.int8)
    g[20, 20:236] = 100; g[235, 20:236] = 100; g[20:236, 20] = 100; g[20:236, 235] = 100
    for _ in range(25):
        x, y = rng.integers(30, 220, 2)
        w, h = rng.integers(1, 12, 2)
        g[y:y + h, x:x + w] = 100
    return g, rng


def _free_poses(g, rng, n, res, ox, oy, lo=-5.0, hi=5.0):
    out = []
    while len(out) < n:
        p = np.array([rng.uniform(lo, hi), rng.uniform(lo, hi), rng.uniform(-math.pi, math.pi)], dtype=np.float32)
        if g[S.cell(float(p[1]), oy, res), S.cell(float(p[0]), ox, res)] == 0:
            out.append(p)
    return np.array(out, dtype=np.float32)


def test_noise_is_stateless_bounded_and_drops_its_share():
    g, rng = _room()
    poses = _free_poses(g, rng, 6, RES, -6.4, -6.4)
    kw = dict(max_range=3.0, noise_amp=0.03, dropout_q16=6554, seed=0xC0FFEE, first_record=40)
    r0, c0 = S.sense_ranges(g, RES, -6.4, -6.4, poses, **kw)
    r1, c1 = S.sense_ranges(g, RES, -6.4, -6.4, poses, **kw)
    assert r0.tobytes() == r1.tobytes() and (c0 == c1).all()
    clean, cc = S.sense_ranges(g, RES, -6.4, -6.4, poses, max_range=3.0)
    both = (c0 >= 0) & (cc >= 0)
    assert both.sum() > 300 and (c0[both] == cc[both]).all()
    # |d' - d| < noise_amp before the rounding to float32 (half an ulp of 3.0 on each side)
    assert (np.abs(r0[both].astype(np.float64) - clean[both].astype(np.float64)) < 0.03 + 2.0 ** -21).all()
    assert (r0[both] != clean[both]).mean() > 0.9
    other, _ = S.sense_ranges(g, RES, -6.4, -6.4, poses, **dict(kw, seed=0xC0FFEF))
    assert other.tobytes() != r0.tobytes()
    # the draws themselves: 2^16 of them, |noise| < 1, the dropout share within 3 sigma of q / 65536
    q = 6554
    draws = [S.draw(0xC0FFEE, rec, beam) for rec in range(363) for beam in range(181)][:1 << 16]
    assert len(draws) == 1 << 16
    u = np.array([d[0] for d in draws], dtype=np.float64) * 2.0 ** -24 - 1.0
    assert u.min() >= -1.0 and u.max() < 1.0 and abs(u.mean()) < 3 * math.sqrt(1 / 6 / 65536)      # triangular: variance 1/6
    share = np.mean([(d[1] & 0xFFFF) < q for d in draws])
    p = q / 65536
    assert abs(share - p) < 3 * math.sqrt(p * (1 - p) / 65536), share
    assert S.noisy(1.0, 0.0, 0, 5, 0, 0) == (1.0, False)
    assert all(S.noisy(1.0, 0.0, 65536, 5, r, 3)[1] for r in range(50))


def test_first_record_makes_one_call_equal_two():
    g, rng = _room()
    poses = _free_poses(g, rng, 8, RES, -6.4, -6.4)
    kw = dict(max_range=1.2, noise_amp=0.02, dropout_q16=3000, seed=99)
    whole, cw = S.sense_ranges(g, RES, -6.4, -6.4, poses, first_record=1000, **kw)
    a, ca = S.sense_ranges(g, RES, -6.4, -6.4, poses[:4], first_record=1000, **kw)
    b, cb = S.sense_ranges(g, RES, -6.4, -6.4, poses[4:], first_record=1004, **kw)
    assert np.concatenate([a, b]).tobytes() == whole.tobytes() and (np.concatenate([ca, cb]) == cw).all()
    shifted, _ = S.sense_ranges(g, RES, -6.4, -6.4, poses[4:], first_record=1000, **kw)
    assert shifted.tobytes() != b.tobytes()


def test_emitted_records_parse(P):
    g, rng = _room()
    poses = _free_poses(g, rng, 3, RES, -6.4, -6.4)
    ranges, _ = S.sense_ranges(g, RES, -6.4, -6.4, poses)
    odo = S.sense_sweeps(P, g, RES, -6.4, -6.4, poses, [1, 2, 1], enc=[5, -6, 7], v2v=[8, 9, 0xFFFFFFFF])
    v0 = S.sense_sweeps(P, g, RES, -6.4, -6.4, poses, [1, 2, 1], odometry=False)
    assert odo.shape == (3, 751) and v0.shape == (3, 743)
    for k in range(3):
        agent, x, y, yaw, enc, v2v, rg = P.unpack_v0_odo(odo[k].tobytes())
        assert (agent, enc, v2v) == ((1, 2, 1)[k], (5, -6, 7)[k], (8, 9, 0xFFFFFFFF)[k])
        assert (np.float32(x), np.float32(y), np.float32(yaw)) == tuple(poses[k]) and rg.tobytes() == ranges[k].tobytes()
        agent, x, y, yaw, rg = P.unpack_v0(v0[k].tobytes())
        assert agent == (1, 2, 1)[k] and rg.tobytes() == ranges[k].tobytes()
        assert odo[k, 25:27].tobytes() == b"\xb5\x00" and v0[k, 17:19].tobytes() == b"\xb5\x00"      # scan_count 181
    pk = S.sense_packets(P, g, RES, -6.4, -6.4, poses, [2, 1, 2], enc=[1, 2, 3], landmark=[0, 4, 5])
    r4, _ = S.sense_ranges(g, RES, -6.4, -6.4, poses, 4)
    assert pk.shape == (3, 42) and S.ranges_of(P, pk).tobytes() == r4.tobytes() and (S.ranges_of(P, odo) == ranges).all()
    rec = pk.view(P.PACKET_DTYPE).reshape(-1)
    assert rec["agent"].tolist() == [2, 1, 2] and rec["lm"].tolist() == [0, 4, 5] and rec["enc"].tolist() == [1, 2, 3]


def test_limits():
    assert S.check_params(0.05, 1.2) and S.check_params(0.05, 12.7) and not S.check_params(0.05, 12.71)
    assert not S.check_params(0.05, 0.0) and not S.check_params(0.05, math.inf) and not S.check_params(0.05, math.nan)
    assert not S.check_params(0.05, 1.2, -0.1) and not S.check_params(0.05, 1.2, 0.0, 65537)
    poses = [[math.nan, 0.0, 0.0], [0.0, math.inf, 0.0], [0.0, 0.0, math.nan], [1e30, 0.0, 0.0]]
    g = empty()
    g[:] = 100
    r, c = S.sense_ranges(g, RES, OX, OY, poses, no_return=-2.0)
    assert (r == -2.0).all() and (c == -1).all()
    assert S.cell(1e12, OX, RES) == S.CLAMP and S.cell(-1e12, OX, RES) == -S.CLAMP and S.cell(1e30, OX, RES) is None


@pytest.mark.parametrize("max_range", [1.2, 3.0])
def test_round_trip_through_update_ray(max_range):
    """Sense a built room, feed every returned range back to the reference's update_ray from the same pose along the same beam,
    and measure how far the cell it marks lies from the cell that was hit.  The range is centre to centre and the beam's own
    angle is not the angle to that centre, so the marked cell may be a neighbour: the largest Chebyshev distance is
    ROUND_TRIP_CELLS, the bound the closed-loop GPU test uses."""
    size, res, ox, oy = 256, 0.05, -6.4, -6.4
    g, rng = _room()
    poses = _free_poses(g, rng, 300, res, ox, oy)
    ranges, cells = S.sense_ranges(g, res, ox, oy, poses, max_range=max_range)
    rx, ry, hx, hy, marked, hit = [], [], [], [], [], []
    for k, p in enumerate(poses):
        x, y = float(p[0]), float(p[1])
        for i, a in enumerate(S.angles(p[2], 181)):
            if cells[k, i] < 0:
                continue
            d = float(ranges[k, i])
            ex, ey = x + d * math.cos(a), y + d * math.sin(a)               # dual_bot_mapper.py:890-891
            rx.append(x); ry.append(y); hx.append(ex); hy.append(ey)
            marked.append((S.cell(ex, ox, res), S.cell(ey, oy, res)))
            hit.append((int(cells[k, i]) % size, int(cells[k, i]) // size))
    marked, hit = np.array(marked), np.array(hit)
    assert len(hit) > 5000                                                  # 9 to 27 thousand
    o = orc.OracleMapper(size, res, ox, oy, 0.0)
    o.update_rays(rx, ry, hx, hy, np.ones(len(rx), dtype=np.uint8))
    mine = np.zeros((size, size), dtype=np.int32)
    np.add.at(mine, (marked[:, 1], marked[:, 0]), 1)
    assert (o.hits == mine).all()                                           # `marked` are the cells update_ray marked
    cheb = np.abs(marked - hit).max(axis=1)
    print(f"R = {max_range}: {len(hit)} hits, Chebyshev distance histogram {np.bincount(cheb).tolist()}")
    assert cheb.max() == ROUND_TRIP_CELLS
    assert 0.1 < (cheb > 0).mean() < 0.3
