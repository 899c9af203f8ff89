"""The dense L D L^T solve shared by the optimisers, alone: orbhip_debug_pose_graph_dense_solve_host runs the pose graphs' solve chain
(k_pg_ldlt in one workgroup, or k_pg_big_* -- the stages of csrc/dense_ldlt_big.h that k_ba_big_* and k_pg4_big_* run too -- over many)
on systems of the sizes at which a blocked factorisation goes wrong: 32-column panels, 256-row workgroups of the rows stage, 64-row
tiles of the trailing update, and the size at which the optimisers change path.

Yardstick (ba_step_model.within_bound, K = 128): max|x_dev - x_ld| <= K (max|x_64 - x_ld| + 2^-52 max|x_ld|), x_ld the same
elimination in numpy longdouble, x_64 in float64 (dense_ldlt_model.py)."""
import numpy as np
import pytest

import ba_step_model as bm
import dense_ldlt_model as dm

pytestmark = pytest.mark.gpu

# size: the seam it straddles
SIZES = [1, 31, 32, 33,         # one panel, ragged and full, one column into the second
         64, 65,                # the second panel
         96, 97,                # the trailing update's first 64-row tile (n - 32 = 64), full and one row over
         287, 288, 289,         # the rows stage's first 256-row workgroup (n - 32 = 256), one row short, full, one row over
         481]                   # the first size that takes the many-workgroup path unforced
CASES = [(n, big) for n in SIZES for big in (0, 1) if n <= 480 or big]


def _solve(ctx, A, rhs, big, fill=np.nan):
    import orbhip
    x = np.full(len(rhs), fill)
    ok = orbhip.debug_pose_graph_dense_solve(ctx, A, rhs, x, force_big=bool(big))
    assert orbhip.lib.orbhip_debug_pose_graph_last_path() == (1 if big or len(rhs) > 480 else 0)
    return ok, x


@pytest.mark.parametrize("n,big", CASES)
def test_solution_within_k_of_float64(gpu_ctx, n, big):
    s = dm.system(n)
    ok, x = _solve(gpu_ctx, s["A"], s["rhs"], big)
    assert ok and np.isfinite(x).all()
    e_dev = np.abs(x.astype(dm.LD) - s["x_ld"]).max()
    e_64 = np.abs(s["x_64"].astype(dm.LD) - s["x_ld"]).max()
    floor = bm.EPS64 * np.abs(s["x_ld"]).max()
    print("n %4d %s  cond %.3g  e_dev %.3g  e_64 %.3g  floor %.3g  ratio %.3g" % (
        n, "many workgroups" if big else "one workgroup  ", s["cond"], float(e_dev), float(e_64), float(floor), float(e_dev / (e_64 + floor))))
    assert bm.within_bound(e_dev, e_64, floor)


@pytest.mark.parametrize("big", [0, 1])
def test_rerun_gives_the_same_bytes(gpu_ctx, big):
    s = dm.system(289)
    ok1, x1 = _solve(gpu_ctx, s["A"], s["rhs"], big)
    ok2, x2 = _solve(gpu_ctx, s["A"], s["rhs"], big)
    assert ok1 and ok2 and x1.tobytes() == x2.tobytes()


@pytest.mark.parametrize("big", [0, 1])
@pytest.mark.parametrize("n", [40, 70])
@pytest.mark.parametrize("k", [0, 35])      # a zero pivot in the first panel; in the second, reached after one trailing update
def test_zero_pivot_is_flagged_and_x_untouched(gpu_ctx, n, k, big):
    # what counts as a failed pivot (ldlt_rows2 / ldlt_diag_step, csrc/ba_ldlt.h): d == 0 or d not finite
    A, rhs = dm.zero_pivot_system(n, k)
    sentinel = -12345.678
    ok, x = _solve(gpu_ctx, A, rhs, big, fill=sentinel)
    assert not ok
    assert (x == sentinel).all()


def test_refuses_bad_sizes(gpu_ctx):
    import orbhip
    C = orbhip.C
    one = np.ones(1)
    ok = C.c_int(7)
    f = orbhip.lib.orbhip_debug_pose_graph_dense_solve_host
    assert f(gpu_ctx.h, one.ctypes.data, 0, one.ctypes.data, one.ctypes.data, 0, C.byref(ok)) == orbhip.E_BADARG
    assert f(gpu_ctx.h, one.ctypes.data, 4097, one.ctypes.data, one.ctypes.data, 0, C.byref(ok)) == orbhip.E_CAPACITY
    assert ok.value == 7 and one[0] == 1.0
