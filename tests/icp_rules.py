"""Built clouds for the registration kernels (csrc/icp.hip: qs_icp) and the yardstick they are judged by.

Plain numpy: no device, no ctypes.  Three parts:

  table()                every row of tests/test_gpu_icp_edges.py: a Row holds the two clouds, max_dist, max_iter and what the
                         row promises to hit (sum blocks, search form, chunk / part counts, sources without a correspondence)
  reference(row)         the loop of icp.hip's header comment, one step at a time.  The nearest-neighbour step is the kernel's
                         own float64 expression (dx*dx + dy*dy on raw coordinates, first minimum by target index; chunked, no
                         n_src x n_dst matrix is held): that step is bit-defined.  Everything after it -- counts, sum d^2,
                         means, the demeaned sums, atan2 / cos / sin, the update, T <- U T, the move of the sources -- runs in
                         np.longdouble.  Every iterate is kept: Ref.T[k], .fitness[k], .rmse[k], .count[k] and the margins.
  admit(ref)             the conditions under which two implementations that differ by rounding must pick the same
                         correspondences and stop at the same iteration; a row that fails one is not comparable at all

Iterate k is the state after k updates (k = 0: the inputs).  Margins of iterate k:
  gap[k]    smallest difference, over the sources, between the distance to the nearest target and to the nearest OTHER
            target (inf with a single target; a bit-identical copy of the nearest target is not another target: the two
            distances tie exactly whatever the rounding of the source, and the lowest index wins in every implementation).  For k >= 1 it must exceed GAP_REL x max(1, max |coordinate|); at k = 0 ties
            are allowed: the inputs are bit-identical and the rule "lowest target index" decides.
  thr[k]    smallest | |d| - max_dist | over the sources: the same bound, every k.
  stop[k]   k >= 1: min(| |d fitness| - 1e-6 |, | |d rmse| - 1e-6 |) must not be below STOP_MARGIN.
  deg[k]    the update taken from iterate k had a degenerate covariance (the rule of include/quasar_slam.h, qs_icp):
            sum |a'|^2 <= 2^-80 n |mean a|^2 or sum |b'|^2 <= 2^-80 n |mean b|^2: its rotation is the identity.
  deg_ratio[k], deg_ratio64[k]   min(sum |a'|^2 / (n |mean a|^2), sum |b'|^2 / (n |mean b|^2)) in long double and in plain
            float64; 0 when a sum is exactly 0, inf when there is no correspondence.
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

L = np.longdouble
REL = 1e-6                           # rel_fitness = rel_rmse (Open3D's defaults, the merge session's)
GAP_REL = 1e-9                       # gap and thr must exceed GAP_REL x max(1, max |coordinate|)
STOP_MARGIN = 1e-8
DEG_THR = 2.0 ** -80                 # the degenerate rule's threshold
DEG_CLEAR = 2.0 ** 20                # genuine rows stay this factor above it
BAR_T = 1e-9                         # clouds within +-13 m: the bars of test_icp_and_voxel_downsample, unchanged
BAR_RMSE = 1e-9
FAR = 1.0e4                          # the offset of the rows far from the origin
# Rows at 1.0e4 m, each on its own: the float64 oracle's distance from the long-double reference (largest over the iterates,
# oracle.icp_planar run with max_iter = k; measured on the CPU, printed again by tests/test_icp_rules_cpu.py) and the device's
# bar: 32 x that, rounded up to one digit.  A tree of 256 followed by a serial sum over blocks is another summation order of
# the same precision, and may sit several times further out.  The moved cloud is judged by the bar of T.
#   row: (oracle T, oracle rmse, bar T, bar rmse)
FAR_BARS = {
    "F-n437_far": (1.83e-10, 2.84e-12, 6e-9, 1e-10),
    "G-n3_single_target_far": (1.21e-12, 2.33e-17, 4e-11, 8e-16),
    "G-n200_single_target_far": (4.11e-11, 2.63e-17, 2e-9, 9e-16),
}

ICP_BLOCK = 256                      # icp.hip: sources per block of the sums, the transform and the scalar search
NNM_ROWS = 128                       # sources per workgroup of the MFMA search (NNM_WAVES x 16 x NNM_ROWT)
NNM_CHUNK = 512                      # targets per LDS stage
MFMA_MIN_DST = 64                    # auto mode: the MFMA search from 64 targets up


# ---- clouds ------------------------------------------------------------------------------------------------------------------
def room():
    """The 437 occupied cells of tests/golden/session_512.npz as grid_to_pcd gives them: row-major, (col, row) * res + origin."""
    g = np.load(os.path.join(GOLDEN, "session_512.npz"), allow_pickle=False)
    rows, cols = np.nonzero(g["grid"] > 50)
    xy = np.stack([cols * 0.05 + -12.8, rows * 0.05 + -12.8], axis=1).astype(np.float64)
    assert len(xy) == 437
    return xy


def room_n(n, seed=None):
    """n points: copies of the room's points in their order, each jittered by +-0.02 m (fixed seed)."""
    r = room()
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    return r[np.arange(n) % len(r)] + rng.uniform(-0.02, 0.02, (n, 2))


def turned(xy, deg, shift=(0.0, 0.0), about=None):
    """xy turned by deg about `about` (default: the origin), then shifted."""
    xy = np.asarray(xy, dtype=np.float64)
    c0 = np.zeros(2) if about is None else np.asarray(about, dtype=np.float64)
    th = np.radians(deg)
    c, s = np.cos(th), np.sin(th)
    return (xy - c0) @ np.array([[c, -s], [s, c]]).T + c0 + np.asarray(shift, dtype=np.float64)


def lattice(nx, ny, pitch):
    j, i = np.mgrid[0:ny, 0:nx]
    return np.stack([i.ravel() * pitch, j.ravel() * pitch], axis=1).astype(np.float64)


def l_shape():
    """60 points along x and 25 along y from the same corner, 0.05 m apart."""
    a = np.stack([np.arange(60) * 0.05, np.zeros(60)], axis=1)
    b = np.stack([np.zeros(25), np.arange(1, 26) * 0.05], axis=1)
    return np.concatenate([a, b])


def line(n, t0=0.0):
    """n points 0.05 m apart along the direction (0.8, 0.6) through (1, -2), the first at parameter t0."""
    t = t0 + np.arange(n) * 0.05
    return np.stack([1.0 + 0.8 * t, -2.0 + 0.6 * t], axis=1)


def around(centre, n, radius, seed):
    rng = np.random.default_rng(seed)
    r = radius * np.sqrt(rng.uniform(0.01, 1.0, n))
    a = rng.uniform(0, 2 * np.pi, n)
    return np.asarray(centre, dtype=np.float64) + np.stack([r * np.cos(a), r * np.sin(a)], axis=1)


# ---- the plan of the MFMA search, restated (icp.hip: nn_prepare, qs_icp_nn_plan) -------------------------------------------------
def nn_plan(n_src, n_dst):
    """(groups, chunks, chunks per part, parts) of the MFMA search."""
    n_pad = (n_dst + 15) // 16 * 16
    groups = (n_src + NNM_ROWS - 1) // NNM_ROWS
    chunks = (n_pad + NNM_CHUNK - 1) // NNM_CHUNK
    parts = (6 * 1024 + groups - 1) // groups
    parts = max(1, min(parts, max(chunks // 8, 1)))
    cpp = (chunks + parts - 1) // parts
    return groups, chunks, cpp, (chunks + cpp - 1) // cpp


def sum_blocks(n_src):
    return (n_src + ICP_BLOCK - 1) // ICP_BLOCK


# ---- rows --------------------------------------------------------------------------------------------------------------------
class Row:
    def __init__(self, group, name, src, dst, max_dist=1.0, max_iter=30, lockstep=False, far=False, nn_modes=False,
                 unmatched=False, iters=None, **promise):
        self.group, self.name, self.key = group, name, f"{group}-{name}"
        self.src = np.ascontiguousarray(src, dtype=np.float64)
        self.dst = np.ascontiguousarray(dst, dtype=np.float64)
        self.max_dist, self.max_iter = max_dist, max_iter
        self.lockstep = lockstep             # the device runs max_iter = k for every k, not only {0, 1, final}
        self.far = far                       # judged by the bars of the rows at 1.0e4 m
        self.nn_modes = nn_modes             # nn_search modes 1 and 2 on the reference's iterate-1 cloud
        self.unmatched = unmatched           # some source has no correspondence at some iterate
        self.iters = iters                   # the reference's iteration count
        self.promise = promise               # blocks=, mfma=, chunks=, parts=, groups=

    @property
    def bars(self):
        return FAR_BARS[self.key][2:] if self.far else (BAR_T, BAR_RMSE)


A_COUNTS = (1, 2, 127, 128, 129, 255, 256, 257, 513)
A_ITERS = {1: 2, 2: 2, 127: 6, 128: 7, 129: 7, 255: 9, 256: 9, 257: 9, 513: 7}
B_COUNTS = (15, 63, 64, 65, 513)
B_ITERS = {15: 7, 63: 11, 64: 10, 65: 12, 513: 9}
SINGLE = (3.35, -7.15)               # the single target of group G
OUTLIERS_MATCHED = 437               # of 497 sources


def _a_src(n):
    return turned(room_n(n), 2.0, (0.06, -0.04))


def _outlier_src(r):
    far = around((r[:, 0].max() + 6.0, r[:, 1].mean()), 60, 0.5, 77)
    return np.concatenate([turned(r, 3.0), far])


_table = None


def table():
    """Every row, built once."""
    global _table
    if _table is not None:
        return _table
    r = room()
    rows = []
    # A. source counts at block and group edges
    for n in A_COUNTS:
        rows.append(Row("A", f"n{n}", _a_src(n), r, lockstep=n <= 257, iters=A_ITERS[n],
                        blocks=sum_blocks(n), mfma=True, groups=(n + 127) // 128, chunks=1, parts=1))
    rows.append(Row("A", "n10241_dst70", _a_src(10241), r[::6][:70], iters=15, unmatched=True,
                    blocks=41, mfma=True, groups=81, chunks=1, parts=1))
    # B. target counts
    src200 = turned(r[::2][:200], 2.0, (0.06, -0.04))
    for n in B_COUNTS:
        rows.append(Row("B", f"dst{n}", src200, room_n(n, 100 + n), nn_modes=n in (63, 64, 65), unmatched=n < 437, iters=B_ITERS[n],
                        blocks=1, mfma=n >= 64, chunks=(n + 511) // 512, parts=1))
    rows.append(Row("B", "dst8200", turned(r[:300], 2.0, (0.06, -0.04)), room_n(8200), iters=27,
                    blocks=2, mfma=True, groups=3, chunks=17, parts=2))
    # the same count of targets, but target j + 4100 is a copy of target j: from j = 508 on the copy lies in the second part,
    # so the parts hand qs_icp_nn_merge_kernel exact ties, at every iterate
    rows.append(Row("B", "dst8200_copies", turned(r[100:400], 2.0, (0.06, -0.04)), np.tile(room_n(4100), (2, 1)), nn_modes=True,
                    iters=29, blocks=2, mfma=True, groups=3, chunks=17, parts=2))
    # C. exact and tie geometry
    lat = lattice(20, 13, 0.05)
    rows.append(Row("C", "room_on_itself", r, r, lockstep=True, nn_modes=True, iters=1, blocks=2, mfma=True, chunks=1, parts=1))
    rows.append(Row("C", "lattice_half_pitch", lat, lat + [0.025, 0.025], lockstep=True, nn_modes=True, iters=3,
                    blocks=2, mfma=True, chunks=1, parts=1))
    rows.append(Row("C", "collinear", line(100, 0.017) + [-0.018, 0.024], line(140, -1.0), lockstep=True, nn_modes=True, iters=2,
                    blocks=1, mfma=True, chunks=1, parts=1))
    # D. large turns
    ls = l_shape()
    rows.append(Row("D", "L_25deg", turned(ls, 25.0), ls, lockstep=True, unmatched=True, iters=3, blocks=1, mfma=True, chunks=1, parts=1))
    rows.append(Row("D", "L_170deg", turned(ls, 170.0, (2.0, 1.0)), ls, max_dist=5.0, lockstep=True, iters=30,
                    blocks=1, mfma=True, chunks=1, parts=1))
    # E. thresholds and outliers
    rows.append(Row("E", "room_1deg_dist008", turned(r, 1.0), r, max_dist=0.08, lockstep=True, unmatched=True, iters=5,
                    blocks=2, mfma=True, chunks=1, parts=1))
    rows.append(Row("E", "outliers", _outlier_src(r), r, lockstep=True, unmatched=True, iters=9,
                    blocks=2, mfma=True, chunks=1, parts=1))
    rows.append(Row("E", "outliers_dist1e3", _outlier_src(r), r, max_dist=1e3, lockstep=True, iters=12,
                    blocks=2, mfma=True, chunks=1, parts=1))
    # F. far from the origin
    rows.append(Row("F", "n437_far", _a_src(437) + FAR, r + FAR, lockstep=True, far=True, iters=8, blocks=2, mfma=True, chunks=1, parts=1))
    # G. degenerate covariance
    one = np.array([SINGLE])
    for n, seed in ((3, 5), (200, 6)):
        s = around(SINGLE, n, 0.4, seed)
        rows.append(Row("G", f"n{n}_single_target", s, one, lockstep=True, iters=2, blocks=1, mfma=False))
        rows.append(Row("G", f"n{n}_single_target_far", s + FAR, one + FAR, lockstep=True, far=True, iters=2, blocks=1, mfma=False))
    rows.append(Row("G", "seven_identical", np.tile(r[100] + [0.013, -0.021], (7, 1)), r, lockstep=True, iters=2,
                    blocks=1, mfma=True, chunks=1, parts=1))
    rows.append(Row("G", "one_source", r[200:201] + [0.011, 0.017], r, lockstep=True, iters=2, blocks=1, mfma=True, chunks=1, parts=1))
    # H. max_iter
    for mi in (0, 1):
        rows.append(Row("H", f"n257_max_iter{mi}", _a_src(257), r, max_iter=mi, lockstep=True, iters=mi,
                        blocks=2, mfma=True, chunks=1, parts=1))
        rows.append(Row("H", f"outliers_max_iter{mi}", _outlier_src(r), r, max_iter=mi, lockstep=True, unmatched=True, iters=mi,
                        blocks=2, mfma=True, chunks=1, parts=1))
    _table = rows
    return rows


def row(key):
    return {r.key: r for r in table()}[key]


# ---- the reference -----------------------------------------------------------------------------------------------------------
def nearest(p, dst, elems=1 << 21):
    """The kernel's search in float64: (index of the first minimum of dx*dx + dy*dy, that minimum, the smallest value among
    the other targets), a block of sources at a time."""
    n = len(p)
    j = np.empty(n, dtype=np.int64); best = np.empty(n); second = np.full(n, np.inf)
    step = max(1, elems // len(dst))
    for lo in range(0, n, step):
        q = p[lo:lo + step]
        dx = q[:, None, 0] - dst[None, :, 0]; dy = q[:, None, 1] - dst[None, :, 1]
        d2 = dx * dx + dy * dy
        jj = d2.argmin(1)                                    # the first minimum
        ar = np.arange(len(q))
        j[lo:lo + step] = jj; best[lo:lo + step] = d2[ar, jj]
        if len(dst) > 1:                                     # bit-identical copies of the nearest target are not "other" targets
            d2[(dst[None, :, 0] == dst[jj, None, 0]) & (dst[None, :, 1] == dst[jj, None, 1])] = np.inf
            second[lo:lo + step] = d2.min(1)
    return j, best, second


def degenerate(saa, sbb, n, am, bm):
    """The rule of qs_icp, on whatever number type the sums have."""
    t = type(saa)(DEG_THR) * n
    return bool(saa <= t * (am[0] * am[0] + am[1] * am[1]) or sbb <= t * (bm[0] * bm[0] + bm[1] * bm[1]))


def _ratio(s, n, m):
    m2 = m[0] * m[0] + m[1] * m[1]
    if s == 0:
        return 0.0
    return float(s / (n * m2)) if m2 > 0 else np.inf


class Ref:
    pass


def run_reference(src, dst, max_dist=1.0, max_iter=30):
    """Every iterate of the loop.  Ref: iters, T [k] (3 x 3 long double), fitness [k] (float: count / n_src as the code
    divides it), rmse [k] (long double), count [k], gap / thr / stop / deg / deg_ratio / deg_ratio64 [k], and of iterate 1
    the cloud as the search sees it (p1), its correspondences (corr1, -1 without) and their squared distances (d2_1)."""
    src = np.ascontiguousarray(src, dtype=np.float64); dst = np.ascontiguousarray(dst, dtype=np.float64)
    dl = dst.astype(L)
    p = src.astype(L)
    n_src = len(src)
    ref = Ref()
    ref.T, ref.fitness, ref.rmse, ref.count = [], [], [], []
    ref.gap, ref.thr, ref.stop, ref.deg, ref.deg_ratio, ref.deg_ratio64 = [], [], [], [], [], []
    ref.scale = max(1.0, float(np.abs(src).max()), float(np.abs(dst).max()))
    ref.p1 = ref.corr1 = ref.d2_1 = None
    max_d2 = max_dist * max_dist

    def evaluate(k):
        p64 = p.astype(np.float64)
        j, best, second = nearest(p64, dst)
        ok = best < max_d2                                   # the kernel's comparison, in float64
        n = int(ok.sum())
        a, b = p[ok], dl[j[ok]]
        d = a - b
        rm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).sum() / L(n)) if n else L(0)
        ref.fitness.append(n / n_src); ref.rmse.append(rm); ref.count.append(n)
        ref.gap.append(float((np.sqrt(second) - np.sqrt(best)).min()))
        ref.thr.append(float(np.abs(np.sqrt(best) - max_dist).min()))
        ref.scale = max(ref.scale, float(np.abs(p64).max()))
        if k == 1:
            ref.p1 = p64
            ref.corr1 = np.where(ok, j, -1).astype(np.int32)
            ref.d2_1 = np.where(ok, best, 0.0)
        return a, b, n, p64[ok], dst[j[ok]]

    T = np.eye(3, dtype=L)
    ref.T.append(T.copy())
    a, b, n, a64, b64 = evaluate(0)
    ref.stop.append(np.inf)
    it = 0
    while it < max_iter:
        U = np.eye(3, dtype=L)
        if n > 0:
            am, bm = a.sum(0) / L(n), b.sum(0) / L(n)
            ac, bc = a - am, b - bm
            dot = (ac[:, 0] * bc[:, 0] + ac[:, 1] * bc[:, 1]).sum()
            cross = (ac[:, 0] * bc[:, 1] - ac[:, 1] * bc[:, 0]).sum()
            saa = (ac[:, 0] * ac[:, 0] + ac[:, 1] * ac[:, 1]).sum()
            sbb = (bc[:, 0] * bc[:, 0] + bc[:, 1] * bc[:, 1]).sum()
            deg = degenerate(saa, sbb, n, am, bm)
            theta = L(0) if deg else np.arctan2(cross, dot)
            c, s = np.cos(theta), np.sin(theta)
            U[0, 0] = c; U[0, 1] = -s; U[1, 0] = s; U[1, 1] = c
            U[0, 2] = bm[0] - (c * am[0] - s * am[1])
            U[1, 2] = bm[1] - (s * am[0] + c * am[1])
            ref.deg.append(deg)
            ref.deg_ratio.append(min(_ratio(saa, n, am), _ratio(sbb, n, bm)))
            # the same sums in plain float64, as the oracle and the device have them up to the order of summation
            am64, bm64 = a64.mean(0), b64.mean(0)
            ac64, bc64 = a64 - am64, b64 - bm64
            ref.deg_ratio64.append(min(_ratio((ac64 * ac64).sum(), n, am64), _ratio((bc64 * bc64).sum(), n, bm64)))
        else:
            ref.deg.append(False); ref.deg_ratio.append(np.inf); ref.deg_ratio64.append(np.inf)
        T = U @ T
        p = np.stack([U[0, 0] * p[:, 0] + U[0, 1] * p[:, 1] + U[0, 2], U[1, 0] * p[:, 0] + U[1, 1] * p[:, 1] + U[1, 2]], axis=1)
        ref.T.append(T.copy())
        it += 1
        a, b, n, a64, b64 = evaluate(it)
        dfit = abs(ref.fitness[it - 1] - ref.fitness[it]); drm = abs(ref.rmse[it - 1] - ref.rmse[it])
        ref.stop.append(float(min(abs(dfit - REL), abs(drm - REL))))
        if dfit < REL and drm < REL:
            break
    ref.iters = it
    ref.src = src
    return ref


_refs = {}


def reference(r):
    """The reference of a row, computed once per process and left unchanged."""
    if r.key not in _refs:
        _refs[r.key] = run_reference(r.src, r.dst, r.max_dist, r.max_iter)
    return _refs[r.key]


def moved(T, src):
    """T applied to the inputs, in long double (so that what is compared is T, not the rounding of the product)."""
    T = np.asarray(T, dtype=L); s = np.asarray(src, dtype=L)
    return np.stack([T[0, 0] * s[:, 0] + T[0, 1] * s[:, 1] + T[0, 2], T[1, 0] * s[:, 0] + T[1, 1] * s[:, 1] + T[1, 2]], axis=1)


def admit(ref):
    """(ok, why): every margin of every iterate."""
    bound = GAP_REL * ref.scale
    for k in range(ref.iters + 1):
        if k >= 1 and not ref.gap[k] > bound:
            return False, f"gap[{k}] = {ref.gap[k]:.3e} <= {bound:.3e}"
        if not ref.thr[k] > bound:
            return False, f"thr[{k}] = {ref.thr[k]:.3e} <= {bound:.3e}"
        if k >= 1 and ref.stop[k] < STOP_MARGIN:
            return False, f"stop[{k}] = {ref.stop[k]:.3e} < {STOP_MARGIN:.0e}"
    return True, ""


def errors(T, rmse, ref, k):
    """(error of T, of rmse, of the moved cloud) against iterate k of the reference."""
    eT = float(np.abs(np.asarray(T, dtype=L) - ref.T[k]).max())
    er = float(abs(L(rmse) - ref.rmse[k]))
    em = float(np.abs(moved(T, ref.src) - moved(ref.T[k], ref.src)).max())
    return eT, er, em
