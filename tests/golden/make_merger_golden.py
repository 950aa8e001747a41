#!/usr/bin/env python3
"""Golden calls of the reference's map merger.  RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference), like make_golden.py.

server_nodes/map_merger.py imports rclpy, nav_msgs and open3d, none of which is installed; what it does with them in
grid_to_pcd, publish_global_map and the control flow of map_callback is plain numpy around a handful of calls.  This script
loads it with stand-in modules (as make_view_golden.py loads the renderer with a stand-in pygame), makes a MapMerger with
object.__new__, gives it a publisher that keeps what it is handed, and writes to merger_calls.npz:

  g<i>_*   grids: data, (res, ox, oy); the points of its own grid_to_pcd; the message of its own publish_global_map on them
  c<i>_*   clouds: points, res; the message of publish_global_map
  q<i>_*   map_callback sequences: per message the grid, what the stand-in registration_icp was told to return, the cloud
           calls in order with their arguments, the message if one was published, and map_resolution / map_origin afterwards

The stand-in cloud holds points and records calls.  transform() keeps its argument and leaves the points alone (every chosen
transformation is the identity), voxel_down_sample() keeps its argument and the points it was called on and returns them
unchanged.  It stands for no Open3D arithmetic: ICP and voxel rounding against Open3D (N3) stay unpinned.

    python tests/golden/make_merger_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)
from npz_fixed import write_npz  # noqa: E402

CALL_ICP, CALL_TRANSFORM, CALL_IADD, CALL_VOXEL, CALL_PUBLISH = 1, 2, 3, 4, 5
CELL_VALUES = np.array([-128, -1, 0, 50, 51, 100, 127], dtype=np.int8)
LOG = []                                   # the cloud calls of the callback that is running


# ---- stand-in modules ------------------------------------------------------------------------------------------------------
class Cloud:
    def __init__(self, pts=None):
        self._p = np.zeros((0, 3)) if pts is None else np.asarray(pts, dtype=np.float64).reshape(-1, 3)

    points = property(lambda self: self._p, lambda self, v: setattr(self, "_p", np.asarray(v, dtype=np.float64).reshape(-1, 3)))

    def is_empty(self):
        return len(self._p) == 0

    def transform(self, T):
        LOG.append((CALL_TRANSFORM, np.array(T, dtype=np.float64), len(self._p)))
        return self

    def __iadd__(self, other):
        LOG.append((CALL_IADD, len(self._p), len(other._p)))
        self._p = np.concatenate([self._p, other._p])
        return self

    def voxel_down_sample(self, voxel_size):
        LOG.append((CALL_VOXEL, float(voxel_size), self._p.copy()))
        return Cloud(self._p.copy())


class IcpResult:
    def __init__(self, fitness, transformation):
        self.fitness, self.transformation = fitness, transformation


ICP_RETURNS = []                           # what the next registration_icp calls return: (fitness, transformation)


def registration_icp(source, target, threshold, trans_init, estimation, criteria):
    fitness, T = ICP_RETURNS.pop(0)
    LOG.append((CALL_ICP, len(source.points), len(target.points), float(threshold), np.array(trans_init), criteria.max_iteration))
    return IcpResult(fitness, T)


def stand_ins():
    rclpy = types.ModuleType("rclpy")
    node = types.ModuleType("rclpy.node")

    class Node:
        def get_clock(self):
            return types.SimpleNamespace(now=lambda: types.SimpleNamespace(to_msg=lambda: 0))

        def get_logger(self):
            return types.SimpleNamespace(warn=lambda *a: None, info=lambda *a: None)

    node.Node = Node
    rclpy.node = node
    nav = types.ModuleType("nav_msgs")
    msg = types.ModuleType("nav_msgs.msg")

    class OccupancyGrid:
        def __init__(self):
            self.header = types.SimpleNamespace(stamp=None, frame_id="")
            self.info = types.SimpleNamespace(resolution=0.0, width=0, height=0, origin=types.SimpleNamespace(
                position=types.SimpleNamespace(x=0.0, y=0.0, z=0.0), orientation=types.SimpleNamespace(w=0.0)))
            self.data = []

    msg.OccupancyGrid, msg.MapMetaData = OccupancyGrid, object
    nav.msg = msg
    o3d = types.ModuleType("open3d")
    o3d.geometry = types.SimpleNamespace(PointCloud=Cloud)
    o3d.utility = types.SimpleNamespace(Vector3dVector=lambda p: np.asarray(p, dtype=np.float64))
    o3d.pipelines = types.SimpleNamespace(registration=types.SimpleNamespace(
        registration_icp=registration_icp, TransformationEstimationPointToPoint=lambda: None,
        ICPConvergenceCriteria=lambda max_iteration: types.SimpleNamespace(max_iteration=max_iteration)))
    sys.modules.update({"rclpy": rclpy, "rclpy.node": node, "nav_msgs": nav, "nav_msgs.msg": msg, "open3d": o3d})
    return OccupancyGrid


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_map_merger", os.path.join(REF, "server_nodes", "map_merger.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Keeper:
    def __init__(self):
        self.kept = []

    def publish(self, msg):
        LOG.append((CALL_PUBLISH,))
        self.kept.append(msg)


def new_merger(ref):
    mm = object.__new__(ref.MapMerger)                     # __init__ (:9-33) needs a running rclpy; its three state lines:
    mm.global_pcd = Cloud()
    mm.map_resolution = 0.05
    mm.map_origin = [0.0, 0.0]
    mm.publisher_ = Keeper()
    return mm


def message(OccupancyGrid, data, res, ox, oy):
    m = OccupancyGrid()
    m.header.frame_id = "map"
    m.info.resolution, m.info.height, m.info.width = float(res), data.shape[0], data.shape[1]
    m.info.origin.position.x, m.info.origin.position.y = float(ox), float(oy)
    m.data = data.reshape(-1).tolist()
    return m


def published(out, key, msg):
    out[key + "_pub_dims"] = np.array([msg.info.height, msg.info.width], dtype=np.int32)
    out[key + "_pub_origin"] = np.array([msg.info.origin.position.x, msg.info.origin.position.y], dtype=np.float64)
    out[key + "_pub_res"] = np.array([msg.info.resolution], dtype=np.float64)
    data = np.array(msg.data, dtype=np.int64)
    assert len(data) == msg.info.height * msg.info.width and set(np.unique(data)) <= {-1, 100}
    out[key + "_pub_data"] = data.astype(np.int8).reshape(msg.info.height, msg.info.width)
    assert msg.header.frame_id == "map_global" and msg.info.origin.orientation.w == 1.0


# ---- the cases -------------------------------------------------------------------------------------------------------------
def grids():
    """(data, res, ox, oy)."""
    rng = np.random.default_rng(20261021)
    out = []
    for (h, w), res, ox, oy in (((7, 13), 0.05, -0.35, 0.2), ((13, 7), 0.1, 1.5, -2.75), ((64, 64), 0.05, -1.6, -1.6),
                                ((33, 5), 0.03, -1234.5, 987.25), ((1, 17), 0.1, 4000.0, -4000.0), ((40, 3), 0.03, -0.7, -0.1)):
        out.append((rng.choice(CELL_VALUES, size=(h, w)), res, ox, oy))
    out.append((np.array([[127]], dtype=np.int8), 0.05, -3.0, 2.0))                  # 1 x 1, occupied
    out.append((np.array([[50]], dtype=np.int8), 0.05, -3.0, 2.0))                   # 1 x 1, 50 is not occupied: empty
    out.append((np.full((9, 4), -1, dtype=np.int8), 0.1, 0.0, 0.0))                  # all unknown: empty
    row = np.full((1, 31), 0, dtype=np.int8); row[0, [0, 30]] = [51, 100]
    out.append((row, 0.03, -0.45, 0.0))                                              # one row, its two ends
    col = np.full((29, 1), -128, dtype=np.int8); col[[3, 28], 0] = 127
    out.append((col, 0.1, 12.5, -12.5))
    return out


def integer_extent(lo, res):
    """The smallest k >= 5 for which ((lo + k * res) - lo) / res is exactly k in doubles."""
    for k in range(5, 400):
        if ((lo + k * res) - lo) / res == float(k):
            return k, lo + k * res
    raise AssertionError((lo, res))


def clouds():
    """(points [n, 2], res, tag)."""
    out = []
    for res, lo in ((0.05, 0.0), (0.1, -3.2), (0.03, 812.75)):
        k, hi = integer_extent(lo, res)
        for tag, top in (("exact", hi), ("above", float(np.nextafter(hi, np.inf))), ("below", float(np.nextafter(hi, -np.inf)))):
            # x spans the extent under test; y holds four points that truncate into one cell and one on the next
            xs = [lo, top, lo + 0.5 * res, lo + 2.25 * res, lo + 2.75 * res]
            ys = [lo + 0.1 * res, lo + 0.2 * res, lo + 0.7 * res, lo + 0.999 * res, lo + 1.5 * res]
            out.append((np.array([xs, ys]).T, res, f"{tag}_k{k}"))
    out.append((np.array([[-7.25, 3.5]]), 0.05, "one_point"))
    out.append((np.array([[1.0, 2.0], [1.0, 2.0]]), 0.1, "two_equal_points"))
    return out


def sequences():
    """[(grid, res, ox, oy, fitness the stand-in ICP returns or None)] per sequence."""
    rng = np.random.default_rng(7)

    def g(h, w, p=0.2):
        return np.where(rng.random((h, w)) < p, np.int8(100), np.int8(-1)).astype(np.int8)

    empty = np.full((6, 6), 0, dtype=np.int8)
    below = float(np.nextafter(0.6, 0.0))
    q0 = [(empty, 0.2, 9.0, 9.0, None),                   # empty before anything: returns, state stays at its defaults
          (g(12, 9), 0.1, -3.2, 1.6, None),               # adopted: resolution and origin of this message
          (g(20, 20), 0.05, -3.0, 1.5, 0.6),              # fitness exactly 0.6: accepted; voxel size and publish at 0.1
          (g(10, 10), 0.05, -2.0, 2.0, below),            # the double below 0.6: rejected, nothing published
          (empty, 0.05, 0.0, 0.0, None),                  # empty after adoption: returns
          (g(15, 11), 0.03, -3.1, 1.7, 1.0)]              # another resolution again: still 0.1
    q1 = [(g(5, 8, 0.5), 0.03, 100.0, -100.0, None),
          (g(5, 8, 0.5), 0.1, 100.0, -100.0, 0.0),        # rejected at once
          (g(7, 7, 0.5), 0.1, 100.1, -100.2, 0.75)]
    return [q0, q1]


def main():
    OccupancyGrid = stand_ins()
    ref = load_reference()
    out = {"cell_values": CELL_VALUES}
    gs = grids()
    seen = set()
    for i, (data, res, ox, oy) in enumerate(gs):
        key = f"g{i}"
        mm = new_merger(ref)
        pcd = mm.grid_to_pcd(message(OccupancyGrid, data, res, ox, oy))
        pts = np.asarray(pcd.points).reshape(-1, 3)
        assert (pts[:, 2] == 0).all()
        out[key + "_data"], out[key + "_geom"], out[key + "_pcd"] = data, np.array([res, ox, oy]), pts[:, :2].copy()
        seen |= set(np.unique(data).tolist())
        mm.global_pcd, mm.map_resolution = pcd, res
        mm.publish_global_map("map")
        assert len(mm.publisher_.kept) == (0 if pcd.is_empty() else 1)
        if mm.publisher_.kept:
            published(out, key, mm.publisher_.kept[0])
        print(key, data.shape, res, "points", len(pts), "published", out.get(key + "_pub_dims"))
    assert seen >= set(CELL_VALUES.tolist())
    assert tuple(out["g0_pub_dims"]) != out["g0_data"].shape               # the ceil(...) + 1 edge
    out["n_grids"] = np.array([len(gs)], dtype=np.int32)
    cs = clouds()
    widths = {}
    for i, (xy, res, tag) in enumerate(cs):
        key = f"c{i}"
        mm = new_merger(ref)
        mm.global_pcd, mm.map_resolution = Cloud(np.column_stack([xy, np.zeros(len(xy))])), res
        mm.publish_global_map("map")
        published(out, key, mm.publisher_.kept[0])
        out[key + "_xy"], out[key + "_res"] = xy, np.array([res])
        widths[(res, tag.split("_")[0])] = int(out[key + "_pub_dims"][1]), tag
        print(key, tag, res, "dims", out[key + "_pub_dims"])
    for res in (0.05, 0.1, 0.03):
        (we, tag), (wa, _), (wb, _) = widths[(res, "exact")], widths[(res, "above")], widths[(res, "below")]
        k = int(tag.split("_k")[1])
        assert we == k + 1 and wa == k + 2 and wb == k + 1, (res, we, wa, wb)      # the width changes by one at the integer
    for i, (_, _, tag) in enumerate(cs):           # the far point lands on index width - 1 only where the extent is the integer:
        last = (out[f"c{i}_pub_data"][:, -1] == 100).any()     # an ulp to either side the last column of the canvas stays unknown
        assert last == (not tag.startswith(("above", "below"))), tag
    out["n_clouds"] = np.array([len(cs)], dtype=np.int32)
    qs = sequences()
    for i, seq in enumerate(qs):
        mm = new_merger(ref)
        for j, (data, res, ox, oy, fit) in enumerate(seq):
            key = f"q{i}_m{j}"
            del LOG[:]
            del mm.publisher_.kept[:]
            if fit is not None:
                ICP_RETURNS.append((fit, np.identity(4)))
            mm.map_callback(message(OccupancyGrid, data, res, ox, oy), 1)
            assert not ICP_RETURNS or mm.global_pcd.is_empty() or (data > 50).sum() == 0
            del ICP_RETURNS[:]
            out[key + "_data"], out[key + "_geom"] = data, np.array([res, ox, oy])
            out[key + "_fitness"] = np.array([np.nan if fit is None else fit])
            out[key + "_calls"] = np.array([c[0] for c in LOG], dtype=np.int32)
            for c in LOG:
                if c[0] == CALL_ICP:
                    assert c[4].shape == (4, 4) and (c[4] == np.identity(4)).all()
                    out[key + "_icp"] = np.array([c[1], c[2], c[3], c[5]], dtype=np.float64)    # n source, n target, threshold, iterations
                elif c[0] == CALL_TRANSFORM:
                    out[key + "_T"] = c[1]
                elif c[0] == CALL_IADD:
                    out[key + "_iadd"] = np.array([c[1], c[2]], dtype=np.int32)                  # n global (left), n local (right)
                elif c[0] == CALL_VOXEL:
                    out[key + "_voxel_size"], out[key + "_voxel_in"] = np.array([c[1]]), c[2][:, :2].copy()
            if mm.publisher_.kept:
                published(out, key, mm.publisher_.kept[0])
            out[key + "_state"] = np.array([mm.map_resolution, mm.map_origin[0], mm.map_origin[1]], dtype=np.float64)
            out[key + "_global"] = np.asarray(mm.global_pcd.points)[:, :2].copy()
            print(key, "calls", out[key + "_calls"].tolist(), "state", out[key + "_state"].tolist())
        out[f"q{i}_n"] = np.array([len(seq)], dtype=np.int32)
    out["n_sequences"] = np.array([len(qs)], dtype=np.int32)
    out["call_codes"] = np.array([CALL_ICP, CALL_TRANSFORM, CALL_IADD, CALL_VOXEL, CALL_PUBLISH], dtype=np.int32)
    path = os.path.join(HERE, "merger_calls.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
