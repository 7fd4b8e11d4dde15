"""GPU tests of the batched Levenberg-Marquardt fit (vp_lm_run, vp_lm_solve) against the CPU yardstick tests/lm_reference.py.

Tolerances.  The solve hook: the scaled solution within 16 D 2^-52 cond_2(C + lambda I), relative in the 2-norm, of np.linalg.solve
(Cholesky's backward-error bound with room for the reference's own rounding).  One iteration on real data:
|y - y_ref|_2 <= cond_2(C_ref + lambda I) 4e-10 |y_ref|_2, the bound of test_covariance_against_the_inverse_of_the_yardstick (the
GPU's F and g are within 2e-10 of the yardstick's in the scales of their sums).  Converged rows: max_k |g_k| / sqrt(F_kk) <= 1e-4
on the free set, by the yardstick's F and g.  Where a test can only read y off theta_trial - theta at theta != 0 (the held-set
cases of the solve hook) the rounding of theta + delta, eps |theta_k| s_k per index in y, is allowed on top and said there; the
bounded comparisons above use theta = 0 or compare two trial points formed alike.  Measured worst ratios: profiles/lm_notes.md."""
import warnings

import numpy as np
import pytest

from conftest import load_golden, LNPROB_RTOL
from helpers import engine_from_fixture
from oracle import voigt_oracle as vo
import lm_reference as lm
from test_gpu_grad import _same_bits
from test_gpu_fisher import _fitter_from_fixture, _inbox
from test_lm_reference import _spd, STATIONARITY, MARGIN

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
LAM0 = lm.DEFAULTS["lambda0"]
_REF = {}                    # name -> (in-box rows, [(lnprob, F, g)]): made once, never modified


def _start_ref(name):
    if name not in _REF:
        z = load_golden(name)
        insts = vo.instruments_from_fixture(z)
        rows = _inbox(z, insts)
        _REF[name] = (rows, [lm.evaluate(t, z["lb"], z["ub"], insts) for t in rows])
    return _REF[name]


def _bounds_engine(lb, ub):
    import rbvfit_amd
    eng = rbvfit_amd.Engine(0)
    eng.set_bounds(lb, ub)
    return eng


# ---- 1. the solve hook against NumPy -------------------------------------------------------------------------------------
def _numpy_rows(D, W):
    """W well-posed systems of D parameters, cond_2(F) from 1 to 1e6, at theta = 0 inside bounds no step reaches."""
    rng = np.random.default_rng(1000 * D + W)
    lb, ub = -np.full(D, 1e9), np.full(D, 1e9)           # no step is clipped: cond <= 1e6 and lambda >= 1e-6 keep |delta| below 1e7
    F = np.array([_spd(rng, D, 10.0 ** rng.uniform(0, 6)) for _ in range(W)])
    g = rng.standard_normal((W, D))
    theta = np.zeros((W, D))                               # theta_trial is the step itself
    lam = np.array([[1e-3, 1.0, 1e-6][w % 3] for w in range(W)])
    return lb, ub, F, g, theta, lam


def _check_against_numpy(F, g, lam, trial, pred, label):
    """The scaled step and pred of every row against np.linalg.solve; returns the worst ratio to the bound."""
    W, D = g.shape
    worst = 0.0
    for w in range(W):
        s = np.sqrt(np.diag(F[w]))
        C = F[w] / np.outer(s, s)
        A = C + lam[w] * np.eye(D)
        y_ref = np.linalg.solve(A, g[w] / s)
        y = trial[w] * s
        bound = 16 * D * EPS * np.linalg.cond(A)
        ratio = np.linalg.norm(y - y_ref) / np.linalg.norm(y_ref) / bound
        worst = max(worst, ratio)
        assert ratio <= 1.0, "%s row %d: |y - y_ref| / |y_ref| = %.3e x the bound" % (label, w, ratio)
        p_ref = (g[w] / s) @ y_ref - 0.5 * y_ref @ C @ y_ref
        assert abs(pred[w] - p_ref) <= 4 * bound * abs(p_ref) + 16 * EPS * abs(p_ref)
    return worst


# D: one lane, below / at / above a wave's 32-lane half, a full wave (64), the two-wave form (96); W: one row, a few, more than a wave of rows
@pytest.mark.parametrize("D", [1, 2, 3, 6, 24, 31, 32, 33, 64, 96])
@pytest.mark.parametrize("W", [1, 5, 70])
def test_solve_against_numpy(D, W):
    lb, ub, F, g, theta, lam = _numpy_rows(D, W)
    with _bounds_engine(lb, ub) as eng:
        trial, pred, held, ok = eng.lm_solve(F, g, theta, lam)
    assert trial.shape == (W, D) and pred.shape == (W,) and held.shape == (W, D) and ok.shape == (W,)
    assert np.all(ok) and not np.any(held)
    worst = _check_against_numpy(F, g, lam, trial, pred, "D=%d W=%d" % (D, W))
    print("D=%d W=%d: worst |y - y_ref|_2 / |y_ref|_2 = %.3f of 16 D eps cond" % (D, W, worst))


def _held_cases():
    """Six rows of D = 6 between two plain ones, every way an index is held (and the two ways a bound does not hold it)."""
    rng = np.random.default_rng(7)
    D = 6
    lb, ub = -np.full(D, 50.0), np.full(D, 50.0)
    F = np.array([_spd(rng, D, 1e3) * np.outer(sc, sc) for sc in 10.0 ** rng.uniform(-1, 1, (8, D))])
    g = rng.standard_normal((8, D))
    theta = rng.uniform(-1, 1, (8, D))
    theta[1, 0], g[1, 0] = lb[0], -1.0                     # lower bound, outward: held
    theta[2, 0], g[2, 0] = lb[0], 1.0                      # lower bound, inward: free
    theta[3, 1], g[3, 1] = ub[1], 1.0                      # upper bound, outward: held
    theta[4, 1], g[4, 1] = ub[1], -1.0                     # upper bound, inward: free
    F[5, 2, :] = 0.0; F[5, :, 2] = 0.0                     # F_kk = 0
    F[6, 3, :] *= 1e-9; F[6, :, 3] *= 1e-9                 # F_kk (ub - lb)^2 < freeze_tol
    want = np.zeros((8, D), dtype=bool)
    want[1, 0] = want[3, 1] = want[5, 2] = want[6, 3] = True
    return lb, ub, F, g, theta, want


def test_solve_held_sets():
    lb, ub, F, g, theta, want = _held_cases()
    lam = np.full(8, LAM0)
    with _bounds_engine(lb, ub) as eng:
        trial, pred, held, ok = eng.lm_solve(F, g, theta, lam)
    assert np.all(ok)
    assert np.array_equal(held, want)
    assert _same_bits(trial[want], theta[want])            # delta_k == 0 exactly
    for w in range(8):
        r = lm.step_full(F[w], g[w], theta[w], lb, ub, LAM0)
        assert np.array_equal(r["held"], want[w]) and r["ok"]
        A = r["C"] + LAM0 * np.eye(r["free"].size)
        y_ref = np.linalg.solve(A, r["gh"])
        y = (trial[w] - theta[w])[r["free"]] * r["s"]
        clipped = (trial[w][r["free"]] == lb[r["free"]]) | (trial[w][r["free"]] == ub[r["free"]])
        # theta + delta rounds at eps |theta|: in y that is eps |theta| s_k
        slack = 2 * EPS * np.linalg.norm(np.maximum(np.abs(theta[w]), np.abs(trial[w]))[r["free"]] * r["s"])
        assert np.linalg.norm((y - y_ref)[~clipped]) <= 16 * 6 * EPS * np.linalg.cond(A) * np.linalg.norm(y_ref) + slack, w
        assert np.all(trial[w] >= lb) and np.all(trial[w] <= ub)
        assert np.array_equal(trial[w][r["free"]][clipped], r["theta_trial"][r["free"]][clipped])


def _held_patterns(D):
    """Rows of D parameters whose held sets come from the four causes of ``_held_cases`` in random places, and the shapes the
    compaction of the free indices can get wrong: no free index, one, the ends held, (D > 64) both sides of the seam of the two waves."""
    rng = np.random.default_rng(4000 + D)
    want = [rng.random(D) < p for p in (0.1, 0.5, 0.9)]                  # random patterns, sparse to dense
    want.append(np.ones(D, dtype=bool))                                  # n = 0
    one = np.ones(D, dtype=bool); one[int(rng.integers(D))] = False      # n = 1
    want.append(one)
    ends = np.zeros(D, dtype=bool); ends[[0, D - 1]] = True
    want.append(ends)
    if D > 64:
        seam = rng.random(D) < 0.2; seam[[62, 63, 64]] = True
        want.append(seam)
        left = np.zeros(D, dtype=bool); left[:64] = True; left[int(rng.integers(64))] = False      # what is free is nearly all in the second wave
        want.append(left)
        right = np.zeros(D, dtype=bool); right[64:] = True               # ... all in the first
        want.append(right)
    want = np.array(want)
    W = len(want)
    lb, ub = -np.full(D, 50.0), np.full(D, 50.0)
    F = np.array([_spd(rng, D, 1e3) * np.outer(sc, sc) for sc in 10.0 ** rng.uniform(-1, 1, (W, D))])
    g = rng.standard_normal((W, D))
    g[g == 0.0] = 1.0
    theta = rng.uniform(-1, 1, (W, D))
    for w in range(W):
        for k in np.nonzero(want[w])[0]:
            cause = int(rng.integers(4))
            if cause == 0:
                theta[w, k], g[w, k] = lb[k], -abs(g[w, k])              # lower bound, outward
            elif cause == 1:
                theta[w, k], g[w, k] = ub[k], abs(g[w, k])               # upper bound, outward
            elif cause == 2:
                F[w, k, :] = 0.0; F[w, :, k] = 0.0                       # F_kk = 0
            else:
                F[w, k, :] *= 1e-9; F[w, :, k] *= 1e-9                   # F_kk (ub - lb)^2 < freeze_tol
        for k in np.nonzero(~want[w])[0][:2]:                            # on a bound with the gradient pointing inward: free
            theta[w, k], g[w, k] = lb[k], abs(g[w, k])
    return lb, ub, F, g, theta, want


# D: above a wave's half, a full wave, one lane into the second wave, the largest
@pytest.mark.parametrize("D", [33, 64, 65, 96])
def test_solve_held_sets_wide(D):
    lb, ub, F, g, theta, want = _held_patterns(D)
    W = len(want)
    lam = np.full(W, LAM0)
    with _bounds_engine(lb, ub) as eng:
        trial, pred, held, ok = eng.lm_solve(F, g, theta, lam)
    assert np.all(ok)
    assert np.array_equal(held, want)
    assert _same_bits(trial[want], theta[want])            # delta_k == 0 exactly
    assert np.all(trial >= lb) and np.all(trial <= ub)
    free_counts = (~want).sum(axis=1).tolist()
    assert 0 in free_counts and 1 in free_counts
    worst = 0.0
    for w in range(W):
        r = lm.step_full(F[w], g[w], theta[w], lb, ub, LAM0)
        assert np.array_equal(r["held"], want[w]) and r["ok"]
        if r["free"].size == 0:                             # every index held: no move, nothing predicted
            assert pred[w] == 0.0 and _same_bits(trial[w], theta[w])
            continue
        A = r["C"] + LAM0 * np.eye(r["free"].size)
        y_ref = np.linalg.solve(A, r["gh"])
        y = (trial[w] - theta[w])[r["free"]] * r["s"]
        clipped = (trial[w][r["free"]] == lb[r["free"]]) | (trial[w][r["free"]] == ub[r["free"]])
        # theta + delta rounds at eps |theta|: in y that is eps |theta| s_k
        slack = 2 * EPS * np.linalg.norm(np.maximum(np.abs(theta[w]), np.abs(trial[w]))[r["free"]] * r["s"])
        bound = 16 * D * EPS * np.linalg.cond(A) * np.linalg.norm(y_ref) + slack
        worst = max(worst, float(np.linalg.norm((y - y_ref)[~clipped]) / bound))
        assert np.linalg.norm((y - y_ref)[~clipped]) <= bound, w
        assert np.array_equal(trial[w][r["free"]][clipped], r["theta_trial"][r["free"]][clipped])
        assert pred[w] > 0.0 and abs(pred[w] - r["pred"]) <= 4 * 16 * D * EPS * np.linalg.cond(A) * r["pred"]
    print("D=%d: free indices per row %s, worst |y - y_ref|_2 = %.3f of its bound" % (D, free_counts, worst))


@pytest.mark.parametrize("D", [6, 64, 96])
def test_solve_is_exact_under_powers_of_two(D):
    """theta_k -> 2^-e_k theta_k, i.e. F' = S F S and g' = S g with S = diag(2^e_k): Marquardt's scaling takes S out again
    without a rounding, so C, gh, y and pred keep their bits and the step is the old one times 2^-e_k.  Bounds of +-1e30: no step
    (at most 1e7 x 2^20) is clipped and no F'_kk (ub - lb)^2 (at least 1e-6 x 2^-40 x 4e60) falls under freeze_tol."""
    _, _, F, g, theta, lam = _numpy_rows(D, 5)
    rng = np.random.default_rng(D)
    S = 2.0 ** rng.integers(-20, 21, size=(5, D))
    F2, g2 = F * S[:, :, None] * S[:, None, :], g * S
    with _bounds_engine(-np.full(D, 1e30), np.full(D, 1e30)) as eng:
        trial, pred, held, ok = eng.lm_solve(F, g, theta, lam)
        trial2, pred2, held2, ok2 = eng.lm_solve(F2, g2, theta, lam)
    assert np.all(ok) and np.all(ok2) and not np.any(held) and not np.any(held2)
    assert np.all(trial != 0.0) and len(np.unique(S)) > 8
    assert _same_bits(trial2 * S, trial) and _same_bits(pred2, pred)


def test_solve_non_finite_input_fails_its_row_only():
    lb, ub, F, g, theta, _ = _held_cases()
    F, g, theta = F[[0, 7, 0, 7, 0, 7]].copy(), g[[0, 7, 0, 7, 0, 7]].copy(), theta[[0, 7, 0, 7, 0, 7]].copy()      # (rows that hold no index)
    F[0, 1, 4] = F[0, 4, 1] = np.nan
    F[1, 2, 5] = F[1, 5, 2] = np.inf
    g[2, 3] = np.nan
    g[3, 0] = np.inf
    F[4, 2, 2] = np.nan                                     # on the diagonal: not F_kk > 0, the index is held
    lam = np.full(6, LAM0)
    with _bounds_engine(lb, ub) as eng:
        trial, pred, held, ok = eng.lm_solve(F, g, theta, lam)
        solo = [eng.lm_solve(F[[w]], g[[w]], theta[[w]], lam[:1]) for w in (4, 5)]
    assert ok.tolist() == [False, False, False, False, True, True]
    assert _same_bits(trial[:4], theta[:4]) and np.all(np.isfinite(pred)) and np.all(pred[:4] == 0.0)
    assert held[4].tolist() == [False, False, True, False, False, False] and not np.any(held[5]) and not np.any(held[:4])
    assert trial[4, 2] == theta[4, 2] and np.all(trial[4, [0, 1, 3, 4, 5]] != theta[4, [0, 1, 3, 4, 5]]) and np.all(trial[5] != theta[5])
    assert np.all(np.isfinite(trial)) and pred[4] > 0.0 and pred[5] > 0.0
    for n, w in enumerate((4, 5)):
        assert _same_bits(trial[w], solo[n][0][0]) and _same_bits(pred[w], solo[n][1][0]) and solo[n][3][0]
    keep = [0, 1, 3, 4, 5]                                  # the row with the NaN on the diagonal is the 5 x 5 system without that index
    r = lm.step_full(F[4][np.ix_(keep, keep)], g[4][keep], theta[4][keep], lb[keep], ub[keep], LAM0)
    A = r["C"] + LAM0 * np.eye(5)
    y = (trial[4] - theta[4])[keep] * r["s"]
    slack = 2 * EPS * np.linalg.norm(np.maximum(np.abs(theta[4]), np.abs(trial[4]))[keep] * r["s"])
    unclipped = (trial[4][keep] != lb[keep]) & (trial[4][keep] != ub[keep])
    assert np.linalg.norm((y - r["y"])[unclipped]) <= 16 * 6 * EPS * np.linalg.cond(A) * np.linalg.norm(r["y"]) + slack


@pytest.mark.parametrize("D", [6, 64, 96])
def test_solve_with_large_and_mixed_damping(D):
    """lambda = 1e12 on every row, then 1e-12 .. 1e12 within one batch: the bound of test_solve_against_numpy."""
    lb, ub, F, g, theta, _ = _numpy_rows(D, 5)
    worst = []
    with _bounds_engine(lb, ub) as eng:
        for lam in (np.full(5, 1e12), np.array([1e-12, 1e-6, 1.0, 1e6, 1e12])):
            trial, pred, held, ok = eng.lm_solve(F, g, theta, lam)
            assert np.all(ok) and not np.any(held)
            worst.append(_check_against_numpy(F, g, lam, trial, pred, "D=%d lambda %g .. %g" % (D, lam[0], lam[-1])))
    print("D=%d: worst |y - y_ref|_2 / |y_ref|_2 = %.3f (lambda 1e12), %.3f (1e-12 .. 1e12) of 16 D eps cond" % (D, worst[0], worst[1]))


def test_solve_indefinite_matrix_fails_its_row_only():
    lb, ub, F, g, theta, _ = _held_cases()
    bad = F[0].copy()
    bad[0, 1] = bad[1, 0] = 3.0 * np.sqrt(bad[0, 0] * bad[1, 1])          # |C_01| = 3: indefinite whatever the rest
    Fb = np.array([F[0], bad, F[7], bad, F[2]])
    gb, tb = g[[0, 0, 7, 7, 2]], theta[[0, 0, 7, 7, 2]]                    # (rows 0 and 7 hold no index: the bad pair stays in the system)
    lam = np.full(5, LAM0)
    with _bounds_engine(lb, ub) as eng:
        trial, pred, held, ok = eng.lm_solve(Fb, gb, tb, lam)
        solo = eng.lm_solve(Fb[[0, 2, 4]], gb[[0, 2, 4]], tb[[0, 2, 4]], lam[:3])
        damped = eng.lm_solve(Fb, gb, tb, np.full(5, 10.0))                # enough damping: every row solves
    assert ok.tolist() == [True, False, True, False, True]
    assert _same_bits(trial[[1, 3]], tb[[1, 3]])                           # a failed row proposes no move
    assert np.all(np.isfinite(trial)) and np.all(np.isfinite(pred))
    assert _same_bits(trial[[0, 2, 4]], solo[0]) and _same_bits(pred[[0, 2, 4]], solo[1])
    assert np.all(damped[3])


def test_solve_refuses_more_than_96_parameters():
    from rbvfit_amd._lib import RbvfitAmdError, VP_EINVAL
    D = 97
    with _bounds_engine(-np.ones(D), np.ones(D)) as eng:
        with pytest.raises(RbvfitAmdError, match="at most 96") as ei:
            eng.lm_solve(np.eye(D)[None], np.ones((1, D)), np.zeros((1, D)), np.ones(1))
        assert ei.value.code == VP_EINVAL and "vp_lm_solve" in str(ei.value)


# ---- 2. one iteration on real data ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c0_mgii", "c3_mini", "dla_lya", "real_cos"])
def test_one_step_against_the_yardstick(name):
    """The scaled step y of EVERY in-box row, accepted or not: the solve hook fed the GPU's own F and g at the row (the inputs and
    the kernel of vp_lm_run's first iteration) against ``lm_reference.step`` fed the yardstick's.  Then vp_lm_run(nsteps=1) itself:
    where the yardstick's accept decision has margin, an accepted row sits at that trial point to the bit, a rejected one has not
    moved and its lambda has doubled.  A row counts as compared when its y was bounded and its decision checked."""
    z = load_golden(name)
    insts = vo.instruments_from_fixture(z)
    lb, ub = z["lb"], z["ub"]
    rows, ref = _start_ref(name)
    with engine_from_fixture(z) as eng:
        _, F_gpu = eng.fisher(rows)
        _, g_gpu = eng.lnprob_grad(rows)
        trial, pred, held, ok = eng.lm_solve(F_gpu, g_gpu, rows, np.full(len(rows), LAM0))
        res = eng.lm_run(rows, nsteps=1)
    assert np.all(ok) and np.all(res.niter == 1) and np.all(np.isin(res.status, (0, 1)))
    used, accepted, worst = 0, 0, 0.0
    for w, t in enumerate(rows):
        lp, F, g = ref[w]
        r = lm.step_full(F, g, t, lb, ub, LAM0)
        assert r["ok"] and np.array_equal(held[w], r["held"]) and _same_bits(trial[w][r["held"]], t[r["held"]])
        A = r["C"] + LAM0 * np.eye(r["free"].size)
        e = (trial[w] - r["theta_trial"])[r["free"]] * r["s"]
        bound = np.linalg.cond(A) * 4e-10 * np.linalg.norm(r["y"])
        worst = max(worst, float(np.linalg.norm(e) / bound))
        assert np.linalg.norm(e) <= bound, "%s row %d: %.3e of the bound" % (name, w, np.linalg.norm(e) / bound)
        assert abs(pred[w] - r["pred"]) <= 4 * np.linalg.cond(A) * 4e-10 * r["pred"]
        lt = vo.lnprob(r["theta_trial"], lb, ub, insts)
        if np.isfinite(lt) and abs(lt - lp) <= MARGIN:
            continue                                        # the accept decision could go either way on rounding
        used += 1
        if np.isfinite(lt) and lt > lp:                     # accepted: the row is at the trial point
            accepted += 1
            assert _same_bits(res.theta[w], trial[w])
            assert abs(res.lnprob[w] - lt) <= LNPROB_RTOL * abs(lt) + 1e-7 and res.lnprob[w] > lp - LNPROB_RTOL * abs(lp)
            assert res.lam[w] < LAM0 * 2
        else:                                               # rejected: the row stays, lambda doubles
            assert _same_bits(res.theta[w], t) and res.lam[w] == LAM0 * 2.0
            assert abs(res.lnprob[w] - lp) <= LNPROB_RTOL * abs(lp)
    print("%s: %d of %d rows compared (%d accepted), worst |y - y_ref|_2 = %.3e of cond 4e-10 |y_ref|_2" % (name, used, len(rows), accepted, worst))
    assert 4 * used >= 3 * len(rows)


# ---- 3. convergence ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c0_mgii", "real_cos"])
def test_convergence(name):
    z = load_golden(name)
    insts = vo.instruments_from_fixture(z)
    lb, ub = z["lb"], z["ub"]
    rows, _ = _start_ref(name)
    with engine_from_fixture(z) as eng:
        start = eng.lm_run(rows, nsteps=0).lnprob
        res = eng.lm_run(rows)
        again = eng.lnprob(res.theta)
    assert np.all(np.isin(res.status, (1, 3))) and np.any(res.status == 1), res.status
    assert np.all(res.lnprob >= start)                      # exact: a row only ever moves to a larger lnprob
    worst = 0.0
    for w in np.nonzero(res.status == 1)[0]:
        t = res.theta[w]
        assert np.all(t >= lb) and np.all(t <= ub)
        assert abs(res.lnprob[w] - again[w]) <= LNPROB_RTOL * abs(again[w])
        _, F, g = lm.evaluate(t, lb, ub, insts)
        st = lm.stationarity(F, g, t, lb, ub)
        worst = max(worst, st)
        assert st <= STATIONARITY, "%s row %d: max |g_k| / sqrt(F_kk) = %.3e" % (name, w, st)
    print("%s: status %s, iterations %s, worst max |g_k| / sqrt(F_kk) = %.3e" % (name, np.bincount(res.status, minlength=4).tolist(),
                                                                                 res.niter.tolist(), worst))


@pytest.mark.parametrize("name", ["c0_mgii", "real_cos"])
def test_best_row_is_no_worse_than_lbfgs(name):
    fit, z, insts, start = _fitter_from_fixture(name)
    try:
        q, _ = fit.fit_quick(grad="analytic")
        lp_q = fit.lnprob(q)
        res = fit.engine.lm_run(_start_ref(name)[0])
    finally:
        fit.close()
    best = res.best()
    assert res.status[best] == 1
    print("%s: lnprob LM best row %.9f, same start %.9f, L-BFGS-B %.9f (difference %.3e)" % (name, res.lnprob[best], res.lnprob[0], lp_q,
                                                                                             res.lnprob[best] - lp_q))
    assert res.lnprob[best] >= lp_q - 1e-6
    assert np.array_equal(_start_ref(name)[0][0], start) and res.status[0] == 1          # ... and so is the row that began at the fitter's start
    assert res.lnprob[0] >= lp_q - 1e-6


# ---- 4. singular directions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c2_window", "c2_mini"])
def test_unconstrained_indices_are_held(name):
    z = load_golden(name)
    lb, ub = z["lb"], z["ub"]
    rows, ref = _start_ref(name)
    width2 = (ub - lb) ** 2
    with engine_from_fixture(z) as eng:
        res = eng.lm_run(rows)
    assert np.all(np.isfinite(res.theta)) and np.all(np.isfinite(res.lnprob)) and np.all(np.isfinite(res.lam))
    assert np.all(np.isfinite(res.fisher)) and np.all(res.status != 2)
    assert np.all(res.theta >= lb) and np.all(res.theta <= ub)
    for w, t in enumerate(rows):
        lp, F, g = ref[w]
        assert res.lnprob[w] >= lp - LNPROB_RTOL * abs(lp)
        # what the data do not constrain at the start nor at the end (by a margin of 1e3 either way of freeze_tol)
        frozen = (np.diag(F) * width2 < 1e-9) & (np.diag(res.fisher[w]) * width2 < 1e-9)
        moved = res.theta[w] != t
        if name == "c2_window":                             # the CIV lines lie outside the spectrum: their b and v say nothing
            assert frozen.tolist() == [k % 8 >= 6 for k in range(24)], np.nonzero(frozen)[0]
        else:                                               # c2_mini: nothing is unconstrained, F is merely ill-conditioned (cond >= 1e12) and
            assert not np.any(frozen)                       # rows run into bounds: whatever did not end on a bound has moved
            assert np.all(moved | (res.theta[w] == lb) | (res.theta[w] == ub)), np.nonzero(~moved)[0]
            assert res.lnprob[w] > lp
        assert _same_bits(res.theta[w][frozen], t[frozen])
        assert np.any(moved) and not np.any(moved & frozen)
    print("%s: status %s, iterations %s" % (name, res.status.tolist(), res.niter.tolist()))


# ---- 5. row isolation, determinism ---------------------------------------------------------------------------------------
def test_bad_rows_get_status_2_and_spare_their_neighbours():
    import rbvfit_amd
    z = load_golden("c0_mgii")
    g_ = lambda k: z["G__" + k]
    lb, ub = z["lb"].copy(), z["ub"].copy()
    D = len(lb)
    lb[D // 3] = 0.0                                        # b = 0 is inside this box: a row there has no finite likelihood
    eng = rbvfit_amd.Engine(0)
    eng.set_bounds(lb, ub)
    eng.add_instrument(g_("wave"), g_("flux"), g_("inv_sigma2"), g_("log_inv_sigma2"), g_("lambda0"), g_("gamma"), g_("f"), g_("zfac"),
                       g_("N_idx"), g_("b_idx"), g_("v_idx"), taps=g_("taps"), lsf_mode=int(g_("lsf_mode")), voigt_method=int(g_("voigt_method")))
    good = _start_ref("c0_mgii")[0][:4]
    out_lo = good[0].copy(); out_lo[0] = lb[0] - 1.0
    out_hi = good[1].copy(); out_hi[D - 1] = ub[D - 1] + 1.0
    nan_row = good[2].copy(); nan_row[3] = np.nan
    b0_row = good[3].copy(); b0_row[D // 3] = 0.0
    bad = {0: out_lo, 2: nan_row, 4: b0_row, 5: out_hi}
    batch = np.array([out_lo, good[0], nan_row, good[1], b0_row, out_hi, good[2]])
    where = [1, 3, 6]
    clean = batch.copy()
    for w in bad:
        clean[w] = good[3]
    with eng:
        lp = eng.lnprob(batch)
        assert not np.any(np.isfinite(lp[list(bad)])) and np.all(np.isfinite(lp[where])), lp
        a = eng.lm_run(batch)
        b = eng.lm_run(batch)
        c = eng.lm_run(clean)
    for w in bad:
        assert a.status[w] == 2 and a.niter[w] == 0
        assert _same_bits(a.theta[w], batch[w])
        assert np.isnan(a.lnprob[w]) and np.isnan(a.lam[w]) and np.all(np.isnan(a.fisher[w]))
    assert np.all(a.status[where] == 1)
    for f in ("theta", "lnprob", "fisher", "lam"):
        assert _same_bits(getattr(a, f), getattr(b, f)), f                                   # the same batch twice
        assert _same_bits(getattr(a, f)[where], getattr(c, f)[where]), f                     # same W, the bad rows replaced
    for f in ("status", "niter"):
        assert np.array_equal(getattr(a, f), getattr(b, f)) and np.array_equal(getattr(a, f)[where], getattr(c, f)[where]), f
    assert np.all(c.status == 1)


def test_non_finite_lnlike_rows_get_status_2():
    import rbvfit_amd
    z = load_golden("c0_mgii")
    g_ = lambda k: z["G__" + k]
    w = g_("inv_sigma2").copy(); lw = g_("log_inv_sigma2").copy()
    w[100] = np.inf; lw[100] = np.inf                                            # error = 0 at one pixel
    bad = rbvfit_amd.Engine(0)
    bad.set_bounds(z["lb"], z["ub"])
    bad.add_instrument(g_("wave"), g_("flux"), w, lw, g_("lambda0"), g_("gamma"), g_("f"), g_("zfac"), g_("N_idx"), g_("b_idx"),
                       g_("v_idx"), taps=g_("taps"), lsf_mode=int(g_("lsf_mode")), voigt_method=int(g_("voigt_method")))
    with bad:
        res = bad.lm_run(z["thetas"], nsteps=3)
    assert np.all(res.status == 2) and np.all(res.niter == 0) and _same_bits(res.theta, z["thetas"])
    assert np.all(np.isnan(res.lnprob)) and np.all(np.isnan(res.fisher)) and np.all(np.isnan(res.lam))


def test_zero_steps_is_the_fisher_entry():
    z = load_golden("c3_mini")
    rows = z["thetas"]
    with engine_from_fixture(z) as eng:
        lp, F = eng.fisher(rows)
        res = eng.lm_run(rows, nsteps=0)
    fin = np.isfinite(lp)
    assert np.any(fin) and np.any(~fin)
    assert res.status.tolist() == [0 if f else 2 for f in fin] and np.all(res.niter == 0)
    assert _same_bits(res.theta, rows)
    assert _same_bits(res.lnprob[fin], lp[fin]) and _same_bits(res.fisher[fin], F[fin])
    assert np.all(np.isnan(res.lnprob[~fin])) and np.all(np.isnan(res.fisher[~fin])) and np.all(np.isnan(F[~fin]))
    assert np.all(res.lam[fin] == LAM0)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,text", [("c0_mgii_fast", "voigt_method 'fast'"), ("nan_wave_gauss", "NaN wavelength"),
                                       ("nan_wave_custom", "NaN wavelength")])
def test_refused_instruments(name, text):
    from rbvfit_amd._lib import RbvfitAmdError, VP_EINVAL
    z = load_golden(name)
    with engine_from_fixture(z) as eng:
        with pytest.raises(RbvfitAmdError, match=text) as ei:
            eng.lm_run(z["thetas"])
        assert ei.value.code == VP_EINVAL and "vp_lm_run" in str(ei.value)
        assert np.array_equal(np.isfinite(eng.lnprob(z["thetas"])),                                # the context stays usable
                              np.isfinite(vo.lnprob_batch(z["thetas"], z["lb"], z["ub"], vo.instruments_from_fixture(z))))


def test_refused_arguments():
    from rbvfit_amd._lib import RbvfitAmdError, VP_EINVAL
    z = load_golden("c0_mgii")
    with engine_from_fixture(z) as eng:
        for kw in (dict(nsteps=-1), dict(lambda0=0.0), dict(lambda0=1.0, lambda_max=0.5), dict(ftol=-1.0), dict(xtol=np.nan)):
            with pytest.raises(RbvfitAmdError, match="nsteps >= 0") as ei:
                eng.lm_run(z["thetas"], **kw)
            assert ei.value.code == VP_EINVAL
        with pytest.raises(TypeError, match="unknown options"):
            eng.lm_run(z["thetas"], gtol=1e-3)
        with pytest.raises(ValueError):
            eng.lm_run(z["thetas"][:, :5])


# ---- 7. vfit -------------------------------------------------------------------------------------------------------------
def test_fit_lm_picks_the_best_row():
    from rbvfit_amd.vfit import covariance_from_fisher
    fit, z, insts, start = _fitter_from_fixture("c0_mgii")
    try:
        q, e = fit.fit_lm(n_starts=8, seed=1)
        res = fit.lm_result
        assert res.theta.shape == (8, 6) and np.any(res.status == 1)
        best = int(np.argmax(np.where(res.status == 1, res.lnprob, -np.inf)))
        assert res.lnprob[best] == np.max(res.lnprob[res.status == 1])
        assert _same_bits(q, res.theta[best]) and _same_bits(fit.theta_best, q) and _same_bits(fit.theta_best_error, e)
        assert _same_bits(fit.theta_best_cov, covariance_from_fisher(res.fisher[best]))
        assert _same_bits(e, np.sqrt(np.diag(fit.theta_best_cov)))
        rng = np.random.default_rng(1)                      # row 0 is the fitter's theta, the others uniform in the box
        starts = np.vstack([start[None, :], rng.uniform(z["lb"], z["ub"], size=(7, 6))])
        q2, _ = fit.fit_lm(starts=starts)
        assert _same_bits(q2, q) and _same_bits(fit.lm_result.theta, res.theta)
        q1, e1 = fit.fit_quick(method="lm")
        assert fit.lm_result.theta.shape == (1, 6) and _same_bits(q1, fit.lm_result.theta[0])
        print("c0_mgii fit_lm: status %s, lnprob %s" % (res.status.tolist(), res.lnprob.tolist()))
    finally:
        fit.close()


def test_fit_quick_defaults_are_what_they_were():
    fit, z, insts, start = _fitter_from_fixture("c0_mgii")
    try:
        q0, e0 = fit.fit_quick()
        assert not hasattr(fit, "theta_best_cov") and not hasattr(fit, "lm_result")
        q1, e1 = fit.fit_quick(method="lbfgs")
        assert _same_bits(q0, q1) and _same_bits(e0, e1)
        assert _same_bits(e0, fit.estimate_parameter_errors(q0, start))
        with pytest.raises(ValueError, match="method must be"):
            fit.fit_quick(method="bogus")
    finally:
        fit.close()


def test_fit_lm_falls_back_on_a_singular_fisher_matrix():
    fit, z, insts, start = _fitter_from_fixture("c2_window")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            q, e = fit.fit_lm(n_starts=1)
        assert any("Fisher errors not available" in str(w.message) for w in rec)
        assert fit.theta_best_cov is None and _same_bits(e, fit.estimate_parameter_errors(q, start))
    finally:
        fit.close()


def test_host_callable_instrument_refused_in_vfit():
    from rbvfit_amd import vfit as mc
    z = load_golden("c0_mgii")
    inst = {"G": {"model": lambda th, wv: np.ones_like(wv), "wave": z["G__wave"], "flux": z["G__flux"],
                  "error": 1.0 / np.sqrt(z["G__inv_sigma2"])}}
    host = mc.vfit(inst, z["theta_true"], z["lb"], z["ub"], no_of_Chain=16, no_of_steps=2)
    try:
        for call in (lambda: host.fit_lm(), lambda: host.fit_quick(method="lm")):
            with pytest.raises(NotImplementedError, match="host-callable"):
                call()
    finally:
        host.close()


# ---- 8. compiler output --------------------------------------------------------------------------------------------------
def test_lm_kernels_use_no_scratch(tmp_path):
    from test_kernel_resources import _metadata
    meta = _metadata(tmp_path)
    mine = {k: v for k, v in meta.items() if k.startswith("vp::lm_")}
    assert sorted(k.split("(")[0] for k in mine) == ["vp::lm_accept_kernel", "vp::lm_init_kernel", "vp::lm_keep_kernel", "vp::lm_mask_kernel",
                                                     "vp::lm_step_kernel"]
    for k, m in mine.items():
        print("%-22s vgpr %3d  sgpr %3d  lds %5d B  scratch %d B  spills v/s %d/%d" % (k.split("(")[0][4:], m["vgpr"], m["sgpr"], m["lds"],
                                                                                       m["scratch"], m["vgpr_spill"], m["sgpr_spill"]))
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, k
