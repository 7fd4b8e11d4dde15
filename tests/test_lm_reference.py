"""CPU tests of the Levenberg-Marquardt yardstick (tests/lm_reference.py), which tests/test_gpu_lm.py holds vp_lm_run to.

(1) ``step`` against np.linalg.solve on the free set, with held indices of every kind; (2) ``run`` on c0_mgii from every in-box
row: converged, stationary in the scaled variables, lnprob never decreasing; (3) the rows the GPU one-step test uses have an
accept decision with margin; (4) the accept rule ``accept`` on hand-made cases; (5) the cases tests/test_gpu_lm_replay.py replays:
the yardstick alone meets the caps that test sets (pairs left out, decisions the oracle can check) and shows the events each case
is there for."""
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


# ---- the accept rule -----------------------------------------------------------------------------------------------------
def test_accept_rule():
    """(lam, nu, lp, lt, pred, ynorm, ok, ftol, xtol, lambda_max) -> (accepted, lam, nu, status); every figure is a power of two or a
    third of one, so the expected values are exact."""
    T = 1.0 / 3.0
    big = 1e12
    cases = [
        # rejections: lambda times nu, nu doubles
        ((1.0, 2.0, 10.0, 9.0, 1.0, 1.0, True, 0.0, 0.0, big), (False, 2.0, 4.0, 0)),
        ((2.0, 4.0, 10.0, 9.0, 1.0, 1.0, True, 0.0, 0.0, big), (False, 8.0, 8.0, 0)),
        ((8.0, 8.0, 10.0, 9.0, 1.0, 1.0, True, 0.0, 0.0, big), (False, 64.0, 16.0, 0)),
        ((1.0, 2.0, 10.0, 10.0, 1.0, 1.0, True, 0.0, 0.0, big), (False, 2.0, 4.0, 0)),           # no gain is no accept
        ((1.0, 2.0, 10.0, np.nan, 1.0, 1.0, True, 0.0, 0.0, big), (False, 2.0, 4.0, 0)),
        ((1.0, 2.0, 10.0, -np.inf, 1.0, 1.0, True, 0.0, 0.0, big), (False, 2.0, 4.0, 0)),
        ((1.0, 2.0, 10.0, np.inf, 1.0, 1.0, True, 0.0, 0.0, big), (False, 2.0, 4.0, 0)),
        ((1.0, 2.0, 10.0, 11.0, 1.0, 0.0, False, 1.0, 1.0, big), (False, 2.0, 4.0, 0)),          # a failed solve: lt, ftol, xtol have no say
        ((4.0, 2.0, 10.0, 9.0, 1.0, 1.0, True, 0.0, 0.0, 8.0), (False, 8.0, 4.0, 0)),            # lambda == lambda_max still runs
        ((4.0, 4.0, 10.0, 9.0, 1.0, 1.0, True, 0.0, 0.0, 8.0), (False, 16.0, 8.0, 3)),           # above it: stalled
        ((4.0, 4.0, 10.0, 9.0, 1.0, 0.5, True, 0.0, 0.5, 8.0), (False, 16.0, 8.0, 1)),           # converged (xtol) wins over stalled
        # accepted steps: rho = gain / pred, lambda times max(1/3, 1 - (2 rho - 1)^3), nu back to 2
        ((3.0, 16.0, 10.0, 11.0, 1.0, 1.0, True, 0.0, 0.0, big), (True, 3.0 * T, 2.0, 0)),       # rho 1: 1/3
        ((3.0, 2.0, 10.0, 12.0, 1.0, 1.0, True, 0.0, 0.0, big), (True, 3.0 * T, 2.0, 0)),        # rho 2: 1 - 27 < 1/3
        ((3.0, 2.0, 10.0, 10.5, 1.0, 1.0, True, 0.0, 0.0, big), (True, 3.0, 2.0, 0)),            # rho 1/2: 1
        ((3.0, 2.0, 10.0, 10.25, 1.0, 1.0, True, 0.0, 0.0, big), (True, 3.0 * 1.125, 2.0, 0)),   # rho 1/4: 1 + 1/8
        ((3.0, 2.0, 8.0, 8.0 + 2.0 ** -40, 2.0 ** 20, 1.0, True, 0.0, 0.0, big), (True, 6.0, 2.0, 0)),      # rho -> 0: 2 (to rounding, below)
        ((3.0, 2.0, 10.0, 10.5, 1.0, 1.0, True, 0.05, 0.0, big), (True, 3.0, 2.0, 1)),           # gain == ftol max(1, |lp|): converged
        ((3.0, 2.0, 10.0, 10.5, 1.0, 1.0, True, 0.04, 0.0, big), (True, 3.0, 2.0, 0)),
        ((3.0, 2.0, 0.25, 0.75, 1.0, 1.0, True, 0.5, 0.0, big), (True, 3.0, 2.0, 1)),            # |lp| < 1: ftol is absolute
        ((3.0, 2.0, 10.0, 10.5, 1.0, 0.25, True, 0.0, 0.25, big), (True, 3.0, 2.0, 1)),          # |y|_inf == xtol: converged
        ((3.0, 2.0, 10.0, 10.5, 1.0, 0.0, True, 0.0, 0.0, big), (True, 3.0, 2.0, 1)),            # every index held
        ((3.0, 2.0, 10.0, 10.5, 1.0, 1.0, True, 0.0, 0.0, 2.0), (True, 3.0, 2.0, 3)),            # an accepted step can stall too
    ]
    for args, want in cases:
        got = lm.accept(*args)
        assert got[0] is want[0] and got[2] == want[2] and got[3] == want[3], (args, got)
        assert abs(got[1] - want[1]) <= 2 * EPS * want[1], (args, got)
    assert lm.accept(*cases[11][0])[1] == 1.0 and lm.accept(*cases[13][0])[1] == 3.0           # the 1/3 branch and u = 0 are exact


def test_ynorm_estimate():
    lb, ub = -np.ones(3), np.ones(3)
    F = np.diag([4.0, 9.0, 16.0])
    none = np.zeros(3, dtype=bool)
    th = np.zeros(3)
    est = lambda trial, held, xtol: lm.ynorm_estimate(np.array(trial), th, F, held, lb, ub, xtol)
    assert est([0.5, 0.1, -0.2], none, 1e-6) == (1.0, True)                                   # max(0.5 x 2, 0.1 x 3, 0.2 x 4)
    assert est([0.0, 0.0, 0.0], ~none, 1e-6) == (0.0, True) and est([0.0, 0.0, 0.0], ~none, 0.0) == (0.0, True)
    assert est([0.5, 0.0, 0.0], np.array([True, False, False]), 1.0) == (0.0, True)           # a held index does not count
    for e, det in ((0.49, True), (0.5, False), (1.0, False), (2.0, False), (2.01, True)):     # within a factor 2 of xtol = 1
        assert lm.ynorm_estimate(np.array([e / 2.0, 0.0, 0.0]), th, F, none, 4.0 * lb, 4.0 * ub, 1.0) == (e, det)
    assert est([0.1, 1.0, 0.0], none, 1.0) == (0.2, False)                                    # clipped and no larger than 2 xtol
    assert est([0.1, -1.0, 0.0], none, 0.01) == (0.2, True)                                   # clipped, the rest already above 2 xtol
    assert est([1.0, 1.0, -1.0], none, 1.0) == (0.0, False)                                   # nothing but clipped indices
    assert est([1.0, 1.0, -1.0], none, 0.0) == (np.finfo(np.float64).tiny, True)              # xtol = 0: always determined


# ---- the cases of tests/test_gpu_lm_replay.py, on the yardstick alone -------------------------------------------------------
# name -> (fixture, rows (None: every in-box row), K (None: the largest niter + 2), options)
REPLAY_CASES = {
    "a": ("c0_mgii", None, None, {}),
    "b": ("c0_mgii", None, 24, dict(ftol=0.0, xtol=0.0, lambda_max=1e3)),
    "c": ("c2_mini", 4, 12, {}),
    "d": ("c2_mini", 4, 16, dict(lambda_max=1e3)),
    "e": ("c3_mini", None, 5, {}),
}
MAX_LEFT_OUT = 0.10          # of a case's (row, iteration) pairs: |y|_inf not determined by its estimate (lm.ynorm_estimate)
MIN_CHECKED = 0.75           # of a case's accept decisions: the oracle's |lnprob_trial - lnprob| > MARGIN
_TRACES = {}


def replay_trace(fixture, nrows, K, opts):
    """The yardstick's iterations of a case -> (K, [(result of run, [one dict per iteration])] per row); made once."""
    key = (fixture, nrows, K, tuple(sorted(opts.items())))
    if key not in _TRACES:
        z, insts, rows = _case(fixture)
        out = []
        for t in rows[:nrows]:
            tr = []
            out.append((lm.run(t, z["lb"], z["ub"], insts, nsteps=50 if K is None else K, trace=tr, **opts), tr))
        _TRACES[key] = (max(r["niter"] for r, _ in out) + 2 if K is None else K, out)
    return _TRACES[key]


def replay_counts(fixture, traces, xtol):
    """Pairs, pairs left out, pairs whose |y|_inf estimate is on the wrong side of xtol, decisions with margin, events."""
    z = load_golden(fixture)
    c = dict(pairs=0, left_out=0, misjudged=0, checked=0, accepted=0, rejected=0, double_reject=0, nu_max=2.0)
    for r, tr in traces:
        live, before = True, True
        for e in tr:
            c["pairs"] += 1
            est, det = lm.ynorm_estimate(e["trial"], e["theta"], e["F"], e["held"], z["lb"], z["ub"], xtol)
            live = live and det
            c["left_out"] += not live
            c["misjudged"] += live and (est <= xtol) != (e["ynorm"] <= xtol)
            c["checked"] += bool(e["ok"] and (not np.isfinite(e["lt"]) or abs(e["lt"] - e["lp"]) > MARGIN))
            c["accepted"] += e["accepted"]
            c["rejected"] += not e["accepted"]
            c["double_reject"] += not e["accepted"] and not before
            before = e["accepted"]
            c["nu_max"] = max(c["nu_max"], e["nu"] if e["accepted"] else 2.0 * e["nu"])
    return c


@pytest.mark.parametrize("case", ["a10", "b10", "c", "d", "e", "real_cos10"])
def test_replay_cases_on_the_yardstick(case):
    """At most 10 % of a case's pairs have an undetermined |y|_inf, and the estimate never lands on the wrong side of xtol where
    it counts as determined; the cases with an oracle check have a margin on at least 75 % of their decisions; every case shows
    the events it is there for.  (c0_mgii and real_cos: their first ten rows here.)"""
    fixture, nrows, K, opts = {"a10": ("c0_mgii", 10, None, {}), "b10": ("c0_mgii", 10, 24, REPLAY_CASES["b"][3]),
                               "real_cos10": ("real_cos", 10, None, {})}.get(case) or REPLAY_CASES[case]
    K, traces = replay_trace(fixture, nrows, K, opts)
    c = replay_counts(fixture, traces, opts.get("xtol", lm.DEFAULTS["xtol"]))
    status = [r["status"] for r, _ in traces]
    print("%s (%s, %d rows, K = %d): %s, status %s" % (case, fixture, len(traces), K, c, status))
    assert c["pairs"] > 0 and c["left_out"] <= MAX_LEFT_OUT * c["pairs"] and c["misjudged"] == 0
    if case in ("a10", "real_cos10"):
        assert all(s == 1 for s in status) and c["rejected"] == 0                 # the defaults never reach the reject branch here
    if case == "b10":
        assert 3 in status and c["nu_max"] >= 8.0 and c["double_reject"] > 0
    if case in ("c", "d", "e"):
        assert c["checked"] >= MIN_CHECKED * c["pairs"]
    if case == "c":
        assert c["accepted"] > 0 and c["rejected"] > 0 and c["double_reject"] > 0
    if case == "d":
        assert 3 in status
