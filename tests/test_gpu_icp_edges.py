"""Registration (csrc/icp.hip: qs_icp) on built clouds: block, group, chunk and part edges, ties, large turns, thresholds,
clouds far from the origin, degenerate covariances, max_iter.

Reference: the long-double restatement of the loop in icp.hip's header (tests/icp_rules.py: reference), computed once per
module; every iterate of it is kept.  Every row meets icp_rules.admit (tests/test_icp_rules_cpu.py): two implementations that
differ by rounding pick the same correspondences and stop at the same iteration, so iterations and fitness are compared with
==.  Bars: T, rmse and the moved source cloud (T applied to the inputs) within 1e-9 for clouds within +-13 m -- the bars of
test_icp_and_voxel_downsample, unchanged.  The rows at 1.0e4 m get 32 x the float64 oracle's own distance from the reference
on the same row, rounded up to one digit (icp_rules.FAR_BARS):

| Row at 1.0e4 m | oracle T | oracle rmse | bar T (and moved cloud) | bar rmse |
| --- | --- | --- | --- | --- |
| F-n437_far | 1.83e-10 | 2.84e-12 | 6e-9 | 1e-10 |
| G-n3_single_target_far | 1.21e-12 | 2.33e-17 | 4e-11 | 8e-16 |
| G-n200_single_target_far | 4.11e-11 | 2.63e-17 | 2e-9 | 9e-16 |

Lock step: the rows of groups C, D, E, F, G, H and the A rows up to 257 sources run with max_iter = k for every k from 0 to the
reference's count and are compared with iterate k; the rest at k in {0, 1, final}.  "Room" is the 437 occupied cells of
tests/golden/session_512.npz, room_n(n) n jittered copies of its points (+-0.02 m, fixed seed); max_dist = 1.0 and max_iter = 30
unless the row says otherwise; turns are about the origin.  Iteration counts in brackets.

| Group | Rows | What they hit |
| --- | --- | --- |
| A. Source counts at block and group edges | room_n(n) turned 2 deg and shifted (0.06, -0.04) against the room, n in {1, 2, 127, 128, 129, 255, 256, 257, 513} [2-9]; 10 241 against 70 room points [15] | The 256-lane tree with a partial last block; one source; 41 blocks in the serial final sum; the 128-row workgroups of the MFMA search |
| B. Target counts | 200 turned room points against room_n(n), n in {15, 63, 64, 65, 513} [7-12; fitness 0.28-0.45 below 437 targets]; 300 sources against room_n(8200) [27]: 17 chunks in 2 parts; 300 against 8 200 targets of which the second 4 100 are copies of the first [29] | The scalar / MFMA switch at 64 targets; the chunk edge at 512; thr_seed across parts on a moving cloud; the corr < 0 branch of every sum; exact ties between the parts in qs_icp_nn_merge_kernel |
| C. Exact and tie geometry | The room against itself [1; rmse 0, T = I exactly]; a 20 x 13 lattice of 0.05 m against itself + (0.025, 0.025) [3]; 100 collinear points against 140 [2] | Ties to the lowest index steering the first update; zero residual; rank-1 covariance |
| D. Large turns | An L (60 + 25 points, 0.05 m apart) turned 25 deg [3]; turned 170 deg, shifted (2, 1), max_dist = 5 [30: the cap] | atan2 outside the small-angle range; the it == max_iter exit; composition over 30 updates |
| E. Thresholds and outliers | The room turned 1 deg with max_dist = 0.08 [5; 401 -> 437 correspondences]; turned 3 deg plus 60 points 6 m away [9; fitness 437 / 497]; the same with max_dist = 1e3 [12] | Correspondences entering; rmse over the inliers only |
| F. Far from the origin | room_n(437) as in A, both clouds + 1.0e4 m [8] | Pass 0 sums raw coordinates; the centring of the MFMA screen |
| G. Degenerate covariance | 3 and 200 sources within 0.4 m of the single target (3.35, -7.15); the same + 1.0e4 m; 7 identical sources near the room; one source [2 each] | The degenerate rule of qs_icp: T[:2, :2] == I exactly on every iterate |
| H. max_iter | A / 257 and E / outliers with max_iter 0 and 1 | it = 0 returns I with the evaluated fitness and rmse |

Rows B / 63-65, B / copies and group C also run nn_search in modes 1 and 2 on the reference's iterate-1 cloud: equal to each other and to
the reference's correspondences, bit for bit."""
import numpy as np
import pytest
import torch  # noqa: F401  before the HIP library: torch bundles its own HIP runtime, and whichever of the two is loaded first has to be torch's

from conftest import load_pkg
import icp_rules as R

pytestmark = pytest.mark.gpu

ROWS = {r.key: r for r in R.table()}
_share = {}


@pytest.fixture(scope="module")
def mapper():
    with load_pkg().QuasarMapper() as m:
        yield m


def steps(r, ref):
    return range(ref.iters + 1) if r.lockstep else sorted({0, min(1, ref.iters), ref.iters})


@pytest.mark.parametrize("key", list(ROWS))
def test_icp_against_the_long_double_reference(mapper, key):
    r = ROWS[key]
    ref = R.reference(r)
    assert ref.iters == r.iters
    bar_t, bar_rm = r.bars
    worst = [0.0, 0.0, 0.0]
    for k in steps(r, ref):
        T, fit, rm, it = mapper.icp(r.src, r.dst, r.max_dist, k)
        e = R.errors(T, rm, ref, k)
        worst = [max(a, b) for a, b in zip(worst, e)]
        print(f"ICP-EDGE {key} k={k}: iterations {it}, fitness {fit!r} (reference {ref.fitness[k]!r}), "
              f"T {e[0]:.2e}, rmse {e[1]:.2e}, moved cloud {e[2]:.2e}")
        assert it == k and fit == ref.fitness[k], (key, k, it, fit, ref.fitness[k])
        assert e[0] <= bar_t and e[1] <= bar_rm and e[2] <= bar_t, (key, k, e)
        assert (T[2] == [0, 0, 1]).all() and T[0, 0] == T[1, 1] and T[0, 1] == -T[1, 0]
        if r.group == "G":
            assert (T[:2, :2] == np.eye(2)).all(), (key, k, T)
        if k == 0:
            assert (T == np.eye(3)).all()
    if r.max_iter > ref.iters:                                        # the stop rule, not the cap, ended the reference
        T, fit, rm, it = mapper.icp(r.src, r.dst, r.max_dist, r.max_iter)
        e = R.errors(T, rm, ref, ref.iters)
        assert it == ref.iters and fit == ref.fitness[-1] and e[0] <= bar_t and e[1] <= bar_rm and e[2] <= bar_t, (key, it, e)
    share = max(worst[0] / bar_t, worst[1] / bar_rm, worst[2] / bar_t)
    g = r.group + (" (1.0e4 m)" if r.far else "")
    _share[g] = max(_share.get(g, 0.0), share)
    print(f"ICP-EDGE {key}: worst T {worst[0]:.2e}, rmse {worst[1]:.2e}, moved cloud {worst[2]:.2e} = {share:.2e} of the bar; "
          f"group {g} so far {_share[g]:.2e}")


@pytest.mark.parametrize("key", [k for k, r in ROWS.items() if r.nn_modes])
def test_search_forms_agree_on_the_moved_cloud(mapper, key):
    r = ROWS[key]
    ref = R.reference(r)
    c1, d1, _ = mapper.nn_search(ref.p1, r.dst, r.max_dist, mode=1)
    c2, d2, _ = mapper.nn_search(ref.p1, r.dst, r.max_dist, mode=2)
    assert np.array_equal(c1, c2) and np.array_equal(d1, d2)
    assert np.array_equal(c1, ref.corr1) and np.array_equal(d1, ref.d2_1)
