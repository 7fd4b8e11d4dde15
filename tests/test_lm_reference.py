"""CPU tests of the Levenberg-Marquardt yardstick (tests/lm_reference.py), which tests/test_gpu_lm.py holds vp_lm_run to.

(1) ``step`` against np.linalg.solve on the free set, with held indices of every kind; (2) ``run`` on c0_mgii from every in-box
row: converged, stationary in the scaled variables, lnprob never decreasing; (3) the rows the GPU one-step test uses have an
accept decision with margin."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import voigt_oracle as vo
import lm_reference as lm

EPS = np.finfo(np.float64).eps
STATIONARITY = 1e-4          # max_k |g_k| / sqrt(F_kk) on the free set, at a converged row
MARGIN = 1e-6                # |lnprob_trial - lnprob| above which an accept decision cannot flip on rounding
_CACHE = {}


def _case(name):
    if name not in _CACHE:
        z = load_golden(name)
        insts = vo.instruments_from_fixture(z)
        rows = [t for t in z["thetas"] if np.isfinite(vo.lnprob(t, z["lb"], z["ub"], insts))]
        _CACHE[name] = (z, insts, rows)
    return _CACHE[name]


def _spd(rng, D, cond):
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    lam = np.exp(rng.uniform(-np.log(cond), 0.0, D))
    lam[0], lam[-1] = 1.0, 1.0 / cond if D > 1 else 1.0
    A = (Q * lam[None, :]) @ Q.T
    return 0.5 * (A + A.T)


@pytest.mark.parametrize("D", [1, 2, 6, 24, 33])
def test_step_against_numpy_solve(D):
    rng = np.random.default_rng(D)
    lb, ub = -np.ones(D) * 50.0, np.ones(D) * 50.0
    for trial in range(6):
        scale = 10.0 ** rng.uniform(-2, 2, D)
        F = _spd(rng, D, 1e4) * np.outer(scale, scale)
        g = rng.standard_normal(D) * scale
        theta = rng.uniform(-1, 1, D)
        lam = [1e-3, 1.0, 1e-6][trial % 3]
        want_held = np.zeros(D, dtype=bool)
        if D >= 6:
            theta[0], g[0] = lb[0], -abs(g[0]); want_held[0] = True          # on the lower bound, gradient outward
            theta[1], g[1] = lb[1], abs(g[1])                                 # ... inward: free
            theta[2], g[2] = ub[2], abs(g[2]); want_held[2] = True            # on the upper bound, outward
            F[3, :] = 0.0; F[:, 3] = 0.0; want_held[3] = True                 # F_kk = 0
            F[4, :] *= 1e-9; F[:, 4] *= 1e-9                                  # F_kk (ub - lb)^2 below freeze_tol
            want_held[4] = F[4, 4] * 1e4 < 1e-6
            assert want_held[4]
        trial_theta, pred, held = lm.step(F, g, theta, lb, ub, lam, 1e-6)
        assert np.array_equal(held, want_held)
        assert np.array_equal(trial_theta[held], theta[held])
        fr_ = np.nonzero(~held)[0]
        s = np.sqrt(np.diag(F)[fr_])
        C = F[np.ix_(fr_, fr_)] / np.outer(s, s)
        gh = g[fr_] / s
        A = C + lam * np.eye(fr_.size)
        y = np.linalg.solve(A, gh)
        full = lm.step_full(F, g, theta, lb, ub, lam, 1e-6)
        assert full["ok"]
        bound = 16 * fr_.size * EPS * np.linalg.cond(A)
        assert np.linalg.norm(full["y"] - y) <= bound * np.linalg.norm(y)
        np.testing.assert_allclose(trial_theta[fr_], np.clip(theta[fr_] + y / s, lb[fr_], ub[fr_]), rtol=0, atol=1e-9 * np.max(np.abs(y / s)))
        assert pred > 0 and abs(pred - (gh @ y - 0.5 * y @ C @ y)) <= 1e-9 * pred
        assert abs(pred - 0.5 * (gh @ y + lam * y @ y)) <= 1e-9 * pred           # the form the kernel evaluates


def test_step_reports_an_indefinite_matrix():
    F = np.array([[1.0, 2.0], [2.0, 1.0]])
    r = lm.step_full(F, np.ones(2), np.zeros(2), -np.ones(2), np.ones(2), 1e-3)
    assert not r["ok"] and np.array_equal(r["theta_trial"], np.zeros(2)) and not np.any(r["held"])
    assert lm.step_full(F, np.ones(2), np.zeros(2), -np.ones(2), np.ones(2), 10.0)["ok"]      # enough damping makes it definite


def test_run_converges_on_c0_mgii():
    z, insts, rows = _case("c0_mgii")
    assert len(rows) >= 8
    worst, most = 0.0, 0
    for t in rows:
        r = lm.run(t, z["lb"], z["ub"], insts)
        assert r["status"] == 1, r
        assert all(b >= a for a, b in zip(r["history"], r["history"][1:]))
        assert r["lnprob"] >= r["history"][0] and r["lnprob"] == r["history"][-1]
        assert np.all(r["theta"] >= z["lb"]) and np.all(r["theta"] <= z["ub"])
        st = lm.stationarity(r["F"], r["g"], r["theta"], z["lb"], z["ub"])
        worst, most = max(worst, st), max(most, r["niter"])
        assert st <= STATIONARITY, st
    print("c0_mgii: %d rows converged, at most %d iterations, worst max |g_k| / sqrt(F_kk) = %.3e" % (len(rows), most, worst))


def test_run_reports_a_start_that_cannot_be_evaluated():
    z, insts, rows = _case("c0_mgii")
    out = rows[0].copy(); out[0] = z["ub"][0] + 1.0
    r = lm.run(out, z["lb"], z["ub"], insts)
    assert r["status"] == 2 and r["niter"] == 0 and np.isnan(r["lnprob"]) and np.array_equal(r["theta"], out)


@pytest.mark.parametrize("name", ["c0_mgii", "c3_mini", "dla_lya", "real_cos"])
def test_first_step_decisions_have_margin(name):
    """tests/test_gpu_lm.py compares one GPU iteration with ``step`` only on rows whose accept decision cannot flip on
    rounding; at most a quarter of a fixture's rows may fall out for that reason."""
    z, insts, rows = _case(name)
    kept = 0
    for t in rows:
        lp, F, g = lm.evaluate(t, z["lb"], z["ub"], insts)
        r = lm.step_full(F, g, t, z["lb"], z["ub"], lm.DEFAULTS["lambda0"])
        assert r["ok"]
        lt = vo.lnprob(r["theta_trial"], z["lb"], z["ub"], insts)
        kept += bool(not np.isfinite(lt) or abs(lt - lp) > MARGIN)
    print("%s: %d of %d rows with margin" % (name, kept, len(rows)))
    assert 4 * kept >= 3 * len(rows)
