"""CPU side of tests/test_gpu_icp_edges.py: every row of its table (tests/icp_rules.py) meets the conditions under which a
registration can be compared at all, hits what its row promises, and the float64 oracle the suite has used so far
(oracle.icp_planar) agrees with the long-double reference on it.

Per row: admit(reference) -- no row is left out: a row that cannot be compared fails here --, the promised sum blocks, search
form, chunk / part counts (icp.hip's qs_icp_nn_plan restated), sources without a correspondence and iteration count; then
oracle.icp_planar with max_iter = k against iterate k of the reference (every k for the lock-step rows, {0, 1, final} for the
rest): iterations and fitness equal, T, rmse and the moved cloud within the row's bars (1e-9 within +-13 m; the rows at
1.0e4 m: icp_rules.FAR_BARS).  Measured, largest per group: T <= 3.9e-14 and rmse <= 3.5e-15 within +-13 m; at 1.0e4 m
T 1.8e-10, rmse 2.8e-12 (group F), T 4.1e-11, rmse 2.6e-17 (group G).

The degenerate rule (include/quasar_slam.h, qs_icp): every update of a G row and of the one-source row of A is degenerate, in
long double and in float64 alike; no update of any other row comes within 2^20 of the threshold (the closest: the room at
1.0e4 m, 3.5e-8 against 2^-80 = 8.3e-25; the G rows: <= 1.3e-29).

What the rule replaced, as a figure: before it, oracle.icp_planar turned the 200 sources around the single target at
(3.35, -7.15) by +1.2474 rad in its first update and by -1.0545 rad over two; the 3 sources by -2.1588 rad; the 200 sources at
+1.0e4 m by -1.4374 rad: atan2 of two sums of rounding noise.  The reference's angle is 0."""
import numpy as np
import pytest

from oracle import oracle as orc
import icp_rules as R

ROWS = {r.key: r for r in R.table()}
_worst = {}


def steps(r, ref):
    return range(ref.iters + 1) if r.lockstep else sorted({0, min(1, ref.iters), ref.iters})


def test_the_table_is_the_issue_s():
    groups = {}
    for r in ROWS.values():
        groups.setdefault(r.group, []).append(r)
    assert sorted(groups) == list("ABCDEFGH")
    assert [len(r.src) for r in groups["A"]] == list(R.A_COUNTS) + [10241] and len(groups["A"][-1].dst) == 70
    assert [len(r.dst) for r in groups["B"]] == list(R.B_COUNTS) + [8200, 8200]
    assert [len(r.src) for r in groups["B"]] == [200] * 5 + [300, 300]
    assert len(R.room()) == 437 and np.abs(R.room()).max() <= 13.0
    assert len(R.l_shape()) == 85 and len(R.lattice(20, 13, 0.05)) == 260
    assert sorted(len(r.src) for r in groups["G"]) == [1, 3, 3, 7, 200, 200]
    assert sorted(r.max_iter for r in groups["H"]) == [0, 0, 1, 1]
    assert sorted(k for k, r in ROWS.items() if r.far) == sorted(R.FAR_BARS)
    for k, (ot, orm, bt, brm) in R.FAR_BARS.items():                     # 32 x the oracle's distance, rounded up to one digit
        for o, b in ((ot, bt), (orm, brm)):
            digit = 10.0 ** np.floor(np.log10(32 * o))
            assert b == pytest.approx(np.ceil(32 * o / digit) * digit, rel=1e-12), (k, o, b)


@pytest.mark.parametrize("key", list(ROWS))
def test_row_is_admitted_and_hits_what_it_claims(key):
    r = ROWS[key]
    ref = R.reference(r)
    ok, why = R.admit(ref)
    print(f"ICP-RULES {key}: iterations {ref.iters}, fitness {min(ref.fitness):.4f}..{max(ref.fitness):.4f}, "
          f"gap {min(ref.gap[1:], default=np.inf):.1e}, thr {min(ref.thr):.1e}, stop {min(ref.stop):.1e}, "
          f"degenerate ratio {min(ref.deg_ratio, default=np.inf):.1e} / fp64 {min(ref.deg_ratio64, default=np.inf):.1e}")
    assert ok, (key, why)
    p = r.promise
    assert R.sum_blocks(len(r.src)) == p["blocks"]
    assert (len(r.dst) >= R.MFMA_MIN_DST) == p["mfma"]
    if p["mfma"]:
        groups, chunks, cpp, parts = R.nn_plan(len(r.src), len(r.dst))
        assert (chunks, parts) == (p["chunks"], p["parts"]) and groups == p.get("groups", groups)
        assert parts * cpp >= chunks > (parts - 1) * cpp
    assert (min(ref.count) < len(r.src)) == r.unmatched
    assert ref.iters == r.iters
    # the degenerate rule: group G and the one-source row through it at every update, nobody else anywhere near it
    expect = r.group == "G" or len(r.src) == 1
    for k in range(ref.iters):
        if ref.count[k] == 0:
            continue
        assert ref.deg[k] == expect, (key, k)
        for ratio in (ref.deg_ratio[k], ref.deg_ratio64[k]):
            if expect:
                assert ratio <= R.DEG_THR
            else:
                assert ratio > R.DEG_THR * R.DEG_CLEAR, (key, k, ratio)
    if r.group == "G":
        for k in range(ref.iters + 1):
            assert (ref.T[k][:2, :2] == np.eye(2)).all()


def test_rows_hit_their_edges():
    """What only some rows promise."""
    ref = R.reference(ROWS["C-room_on_itself"])
    assert ref.iters == 1 and ref.rmse[1] == 0 and (ref.T[1] == np.eye(3)).all()
    r = ROWS["C-lattice_half_pitch"]                                   # four equidistant targets at k = 0, up to the rounding
    d2 = ((r.src[:, None, :] - r.dst[None, :, :]) ** 2).sum(-1)        # of the coordinates: the first minimum decides
    assert ((d2 < d2.min(1, keepdims=True) * (1 + 1e-9)).sum(1) == 4).sum() >= 19 * 12
    assert R.reference(r).gap[0] < 1e-12
    r = ROWS["C-collinear"]                                            # rank 1: both clouds on one line
    for xy in (r.src, r.dst):
        assert np.linalg.svd(xy - xy.mean(0), compute_uv=False)[1] < 1e-12
    ref = R.reference(ROWS["D-L_170deg"])                              # the cap, not convergence
    assert ref.iters == 30 and not (abs(ref.fitness[30] - ref.fitness[29]) < R.REL and abs(ref.rmse[30] - ref.rmse[29]) < R.REL)
    assert abs(np.arctan2(float(ref.T[1][1, 0]), float(ref.T[1][0, 0]))) > 0.1          # outside the small-angle range
    ref = R.reference(ROWS["E-room_1deg_dist008"])                     # correspondences enter
    assert ref.count[0] < ref.count[-1] == 437
    ref = R.reference(ROWS["E-outliers"])
    assert set(ref.count) == {R.OUTLIERS_MATCHED} and ref.fitness[-1] == 437 / 497
    assert set(R.reference(ROWS["E-outliers_dist1e3"]).count) == {497}
    for n in (15, 63, 64, 65):                                         # sources enter and leave between the iterates
        assert len(set(R.reference(ROWS[f"B-dst{n}"]).count)) > 1
    assert R.nn_plan(300, 8200) == (3, 17, 9, 2)                       # the second part starts at target 9 x 512 = 4608
    r = ROWS["B-dst8200_copies"]
    assert np.array_equal(r.dst[:4100], r.dst[4100:])
    c = R.reference(r).corr1                                           # the lowest index wins; most winners' copies lie in part 2
    assert (c >= 0).all() and (c < 4100).all() and ((c >= 508) & (c < 4100)).sum() > 100
    for mi in (0, 1):
        ref = R.reference(ROWS[f"H-n257_max_iter{mi}"])
        assert ref.iters == mi and (mi or (ref.T[0] == np.eye(3)).all()) and ref.rmse[0] > 0.01


@pytest.mark.parametrize("key", list(ROWS))
def test_oracle_agrees_with_the_long_double_reference(key):
    r = ROWS[key]
    ref = R.reference(r)
    bar_t, bar_rm = r.bars
    worst = [0.0, 0.0, 0.0]
    for k in steps(r, ref):
        T, fit, rm, it = orc.icp_planar(r.src, r.dst, r.max_dist, k)
        assert it == k and fit == ref.fitness[k], (key, k, it, fit, ref.fitness[k])
        e = R.errors(T, rm, ref, k)
        worst = [max(a, b) for a, b in zip(worst, e)]
        if r.group == "G":
            assert (T[:2, :2] == np.eye(2)).all()
    g = _worst.setdefault(r.group + ("-far" if r.far else ""), [0.0, 0.0, 0.0])
    g[:] = [max(a, b) for a, b in zip(g, worst)]
    print(f"ICP-RULES {key}: oracle vs long double: T {worst[0]:.2e}, rmse {worst[1]:.2e}, moved cloud {worst[2]:.2e} "
          f"(bars {bar_t:.0e}, {bar_rm:.0e}); largest of group so far: T {g[0]:.2e}, rmse {g[1]:.2e}")
    assert worst[0] <= bar_t and worst[1] <= bar_rm and worst[2] <= bar_t
