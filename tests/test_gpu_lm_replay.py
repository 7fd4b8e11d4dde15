"""GPU tests of vp_lm_run's driver: every iteration replayed through the library's own hooks, the options, the batch shapes.

The replay.  With res_k = Engine.lm_run(rows, nsteps=k), iteration k of the loop is rebuilt from the GPU's own res_{k-1}:
F = Engine.fisher(theta_{k-1}), g = Engine.lnprob_grad(theta_{k-1}), the trial point by Engine.lm_solve(F, g, theta_{k-1},
lam_{k-1}), its lnprob by Engine.lnprob -- the kernels of the loop on the bits of the loop -- and the decision by
``lm_reference.accept``.  So the comparison is exact: theta_k, lnprob_k, niter_k, status_k to the bit; lam_k within 16 x 2^-52
relative (lam' = lam max(1/3, 1 - u^3): exact where the 1/3 wins, elsewhere u^3 carries two roundings against pow's one and
1 - u^3 amplifies them by |u^3| / (1 - u^3) <= 2; a compiler may also contract 1 - u u u into an fma).  The GPU's lam_k is carried
forward, nu is tracked here (2 after an accept, doubled by a reject).  Rows that have finished stay as they are, to the bit, and
every res_k.fisher is Engine.fisher(res_k.theta) to the bit.

vp_lm_solve does not return |y|_inf; ``lm_reference.ynorm_estimate`` reads it off the trial point and says where that cannot
decide the xtol test.  Such a (row, k) pair and the row's later pairs are left out, at most 10 % of a case's pairs;
tests/test_lm_reference.py shows that the yardstick alone keeps to that (it leaves out none), and to the 75 % of decisions that the
oracle check of cases (c), (d), (e) must reach.  The replay rests on a row's F, g and lnprob bits not depending on which other
rows of the batch are evaluated.

Measured event counts and worst ratios: profiles/lm_notes.md."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden, ROOT
from helpers import engine_from_fixture
from oracle import voigt_oracle as vo
import lm_reference as lm
from test_gpu_grad import _same_bits
from test_lm_reference import MARGIN, REPLAY_CASES, MAX_LEFT_OUT, MIN_CHECKED, replay_trace, _case

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
LAM_RTOL = 16 * EPS
FIELDS = ("theta", "lnprob", "fisher", "lam")
COUNTS = ("status", "niter")


def _rows(name):
    """The fixture's in-box rows."""
    return np.array(_case(name)[2])


def _bits_equal(a, b, rows, label):
    for f in FIELDS:
        assert _same_bits(getattr(a, f)[rows], getattr(b, f)[rows]), label + ": " + f
    for f in COUNTS:
        assert np.array_equal(getattr(a, f)[rows], getattr(b, f)[rows]), label + ": " + f


def _replay(eng, z, rows, K, opts, oracle):
    """Replays K iterations; returns (the last result, the event counts)."""
    lb, ub = z["lb"], z["ub"]
    o = dict(lm.DEFAULTS, **opts)
    insts = vo.instruments_from_fixture(z) if oracle else None
    W = len(rows)
    prev = eng.lm_run(rows, nsteps=0, **opts)
    assert np.all(prev.status == 0) and np.all(prev.niter == 0) and np.all(prev.lam == o["lambda0"]) and _same_bits(prev.theta, rows)
    F = eng.fisher(prev.theta)[1]
    assert _same_bits(prev.fisher, F)
    nu = np.full(W, 2.0)
    live = np.ones(W, dtype=bool)                           # no undetermined pair so far
    rejected_before = np.zeros(W, dtype=bool)
    c = dict(pairs=0, left_out=0, accepted=0, rejected=0, double_reject=0, nu_max=2.0, decisions=0, checked=0, worst_lam=0.0)
    lp_oracle = {}
    for k in range(1, K + 1):
        cur = eng.lm_run(rows, nsteps=k, **opts)
        running = prev.status == 0
        _bits_equal(cur, prev, ~running, "k=%d: a finished row changed" % k)
        g = eng.lnprob_grad(prev.theta)[1]
        trial, pred, held, ok = eng.lm_solve(F, g, prev.theta, prev.lam)
        trial[~running] = prev.theta[~running]              # (the loop proposes no move for a finished row)
        lt = eng.lnprob(trial)
        for w in np.nonzero(running)[0]:
            tag = "k=%d row %d" % (k, w)
            c["pairs"] += 1
            est, determined = lm.ynorm_estimate(trial[w], prev.theta[w], F[w], held[w], lb, ub, o["xtol"])
            live[w] = live[w] and determined
            if not live[w]:
                c["left_out"] += 1
                continue
            accepted, lam, nu[w], status = lm.accept(prev.lam[w], nu[w], prev.lnprob[w], lt[w], pred[w], est, ok[w], o["ftol"], o["xtol"],
                                                     o["lambda_max"])
            assert _same_bits(cur.theta[w], trial[w] if accepted else prev.theta[w]), tag
            assert _same_bits(cur.lnprob[w], lt[w] if accepted else prev.lnprob[w]), tag
            assert cur.niter[w] == prev.niter[w] + 1 == k and cur.status[w] == status, (tag, cur.niter[w], cur.status[w], status)
            err = abs(cur.lam[w] - lam) / lam
            c["worst_lam"] = max(c["worst_lam"], err / LAM_RTOL)
            assert err <= LAM_RTOL, "%s: lam %r against %r" % (tag, cur.lam[w], lam)
            c["accepted" if accepted else "rejected"] += 1
            c["double_reject"] += bool(not accepted and rejected_before[w])
            rejected_before[w] = not accepted
            c["nu_max"] = max(c["nu_max"], nu[w])
            if oracle:                                      # where the oracle's two lnprobs are apart, the decision has its sign
                c["decisions"] += 1
                for t in (trial[w], prev.theta[w]):
                    if t.tobytes() not in lp_oracle:
                        lp_oracle[t.tobytes()] = vo.lnprob(t, lb, ub, insts)
                a, b = lp_oracle[trial[w].tobytes()], lp_oracle[prev.theta[w].tobytes()]
                if ok[w] and (not np.isfinite(a) or abs(a - b) > MARGIN):
                    c["checked"] += 1
                    assert accepted == bool(np.isfinite(a) and a > b), "%s: oracle lnprob %r -> %r, accepted %s" % (tag, b, a, accepted)
        F = eng.fisher(cur.theta)[1]
        assert _same_bits(cur.fisher, F), "k=%d: fisher is not that of theta" % k
        prev = cur
    assert c["pairs"] > 0 and c["left_out"] <= MAX_LEFT_OUT * c["pairs"], c
    if oracle:
        assert c["checked"] >= MIN_CHECKED * c["decisions"], c
    return prev, c


@pytest.mark.parametrize("case", sorted(REPLAY_CASES))
def test_replay(case):
    name, nrows, K, opts = REPLAY_CASES[case]
    z = load_golden(name)
    rows = _rows(name)[:nrows]
    if K is None:                                           # (a): the yardstick's largest niter + 2
        K = replay_trace(name, nrows, K, opts)[0]
    with engine_from_fixture(z) as eng:
        res, c = _replay(eng, z, rows, K, opts, oracle=case in "cde")
        dflt = eng.lm_run(rows, nsteps=K) if opts else res
    print("(%s) %s, %d rows, K = %d, %s: %s; status %s, niter %s" % (case, name, len(rows), K, opts or "defaults", c,
                                                                      np.bincount(res.status, minlength=4).tolist(), res.niter.tolist()))
    if case == "a":
        assert np.all(res.status == 1)
    if case == "b":
        assert np.any(res.status == 3) and c["nu_max"] >= 8.0
        assert np.all(dflt.status == 1)                     # ftol, xtol and lambda_max reach the kernel: the defaults end otherwise
    if case == "c":
        assert c["accepted"] > 0 and c["rejected"] > 0 and c["double_reject"] > 0
    if case == "d":
        # the yardstick stalls a row within K (tests/test_lm_reference.py asserts it): so must the GPU
        assert np.any(res.status == 3) and np.any(dflt.status != res.status)   # lambda_max reaches the kernel


# ---- options ---------------------------------------------------------------------------------------------------------------
def test_lambda0_reaches_the_kernel():
    z = load_golden("c3_mini")
    with engine_from_fixture(z) as eng:
        res = eng.lm_run(z["thetas"], nsteps=0, lambda0=0.25)
    assert np.any(res.status == 0) and np.any(res.status == 2)
    assert np.all(res.lam[res.status == 0] == 0.25) and np.all(np.isnan(res.lam[res.status == 2]))


def test_freeze_tol_reaches_the_kernel():
    """c2_window: the CIV lines lie outside the spectrum, F_kk (ub - lb)^2 of their b and v is 4e-32 .. 2e-15.  By default they are
    held; with freeze_tol = 0 whichever of them has F_kk > 0 is free and moves with the first accepted step.  The held set is
    ``lm_reference.held_set`` on the GPU's own F and g."""
    z = load_golden("c2_window")
    lb, ub = z["lb"], z["ub"]
    rows = _rows("c2_window")
    with engine_from_fixture(z) as eng:
        F = eng.lm_run(rows, nsteps=0).fisher
        g = eng.lnprob_grad(rows)[1]
        moved = {ft: eng.lm_run(rows, nsteps=1, freeze_tol=ft).theta != rows for ft in (0.0, 1e-6)}
    outside = np.array([k % 8 >= 6 for k in range(24)])
    for ft in (0.0, 1e-6):
        stepped = np.any(moved[ft], axis=1)                 # (a rejected first step leaves the row where it was)
        assert np.any(stepped)
        for w in np.nonzero(stepped)[0]:
            held = lm.held_set(F[w], g[w], rows[w], lb, ub, ft)
            assert np.array_equal(moved[ft][w], ~held), (ft, w, np.nonzero(moved[ft][w] == held)[0])
            if ft == 0.0:
                assert np.array_equal(held, ~(np.diag(F[w]) > 0))
                assert np.any(~held & outside)
            else:
                assert np.array_equal(held, outside)
    both = np.any(moved[0.0], axis=1) & np.any(moved[1e-6], axis=1)
    assert np.any(both) and np.all(np.any(moved[0.0][both] != moved[1e-6][both], axis=1))


# ---- batch shapes ----------------------------------------------------------------------------------------------------------
_BASE = {}


def _base(eng, name, **kw):
    """The fixture's in-box rows as one batch: what every row of a tiled batch is held to, to the bit."""
    if name not in _BASE:
        rows = _rows(name)
        _BASE[name] = (rows, eng.lm_run(rows, **kw))
    return _BASE[name]


def _tiled_matches(res, base, src, bad, starts, label):
    good = np.ones(len(src), dtype=bool)
    good[list(bad)] = False
    for f in FIELDS:
        assert _same_bits(getattr(res, f)[good], getattr(base, f)[src[good]]), label + ": " + f
    for f in COUNTS:
        assert np.array_equal(getattr(res, f)[good], getattr(base, f)[src[good]]), label + ": " + f
    for w in bad:
        assert res.status[w] == 2 and res.niter[w] == 0 and _same_bits(res.theta[w], starts[w]), (label, w)
        assert np.isnan(res.lnprob[w]) and np.isnan(res.lam[w]) and np.all(np.isnan(res.fisher[w])), (label, w)


# one row; below, at and above the 256 lanes the one-workgroup kernels stride over; more than two strides
@pytest.mark.parametrize("W", [1, 255, 256, 257, 600])
def test_batch_shapes(W):
    z = load_golden("c0_mgii")
    with engine_from_fixture(z) as eng:
        rows, base = _base(eng, "c0_mgii")
        assert np.all(base.status == 1)
        src = np.arange(W) % len(rows)
        starts = rows[src].copy()
        bad = sorted({p for p in (0, 255, 256, W - 1) if p < W})
        for n, p in enumerate(bad):                          # an out-of-box row and a NaN row, in turn
            if n % 2 == 0:
                starts[p, 0] = z["ub"][0] + 1.0
            else:
                starts[p, 3] = np.nan
        res = eng.lm_run(starts)
        _tiled_matches(res, base, src, bad, starts, "W=%d" % W)
        if W == 1:                                          # ... and the one row as a good one
            _tiled_matches(eng.lm_run(rows[:1]), base, src, [], rows[:1], "W=1, in the box")


def test_batch_of_several_fisher_passes():
    """c2_mini with more rows than one pass of the Fisher evaluation takes (2^25 doubles of derivative rows or of partial blocks),
    so that the masked evaluation inside the loop is split: two iterations, every row to the bit of the base batch's."""
    z = load_golden("c2_mini")
    D = len(z["lb"])
    P = max(len(z[str(i) + "__wave"]) for i in z["instruments"])
    with open(os.path.join(ROOT, "rbvfit_amd", "csrc", "fisher_kernels.h")) as f:
        chunk = int(re.search(r"constexpr int FISHER_CHUNK = (\d+);", f.read()).group(1))
    per_pass = 2 ** 25 // max(D * P, -(-P // chunk) * D * D)
    W = per_pass + 3
    assert W <= 2048, W
    with engine_from_fixture(z) as eng:
        rows, base = _base(eng, "c2_mini", nsteps=2)
        src = np.arange(W) % len(rows)
        res = eng.lm_run(rows[src], nsteps=2)
    assert np.all(base.niter == 2) and np.any(base.theta != rows)
    _tiled_matches(res, base, src, [], rows[src], "W=%d (%d rows per pass)" % (W, per_pass))
