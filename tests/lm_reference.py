"""CPU yardstick for the batched Levenberg-Marquardt fit (a helper, not a test): NumPy on top of ``fisher_reference`` and
``grad_reference``.  One row at a time; the rules are those of ``vp_lm_run``.

    maximise lnprob:  lnprob(theta + d) ~ lnprob + g^T d - 1/2 d^T F d,   F = sum_inst J^T W J,  g = d lnprob / d theta

``step(F, g, theta, lb, ub, lam, freeze_tol) -> (theta_trial, pred, held)``:
    held_k  = (theta_k == lb_k and g_k < 0) or (theta_k == ub_k and g_k > 0) or not F_kk > 0 or F_kk (ub_k - lb_k)^2 < freeze_tol
    on the free set, with s = sqrt(diag F):  C = F / (s s^T),  gh = g / s,  (C + lam I) y = gh  (Cholesky),  d = y / s
    theta_trial = clip(theta + d, lb, ub)  (held: theta_k itself),   pred = gh^T y - 1/2 y^T C y
``step_full`` returns the same with y, the free indices, s and ``ok`` (False: C + lam I is not positive definite; theta_trial is
theta then).

``run(theta0, lb, ub, instruments, ...)``: the whole fit of one row, with Nielsen's rule for lam and the status codes
0 running / out of iterations, 1 converged, 2 start not evaluable, 3 stalled (lam > lambda_max).  The rule of one iteration is
``accept(lam, nu, lp, lt, pred, ynorm, ok, ftol, xtol, lambda_max) -> (accepted, lam, nu, status)``, a pure function that ``run``
calls and that tests/test_gpu_lm_replay.py holds every iteration of ``vp_lm_run`` to; ``ynorm_estimate`` is that test's stand-in
for the |y|_inf the solve hook does not return.
"""
import numpy as np

from oracle import voigt_oracle as vo
import grad_reference as gr
import fisher_reference as fr

DEFAULTS = dict(lambda0=1e-3, lambda_max=1e12, ftol=1e-10, xtol=1e-6, freeze_tol=1e-6)


def held_set(F, g, theta, lb, ub, freeze_tol=1e-6):
    d = np.diag(F)
    width = ub - lb
    return ((theta == lb) & (g < 0)) | ((theta == ub) & (g > 0)) | ~(d > 0) | (d * width * width < freeze_tol)


def step_full(F, g, theta, lb, ub, lam, freeze_tol=1e-6):
    F, g, theta, lb, ub = (np.asarray(v, dtype=np.float64) for v in (F, g, theta, lb, ub))
    held = held_set(F, g, theta, lb, ub, freeze_tol)
    free = np.nonzero(~held)[0]
    out = dict(held=held, free=free, ok=True, theta_trial=theta.copy(), pred=0.0, y=np.zeros(free.size), s=np.ones(free.size),
               C=np.zeros((free.size, free.size)), gh=np.zeros(free.size))
    if free.size == 0:
        return out
    s = np.sqrt(np.diag(F)[free])
    C = F[np.ix_(free, free)] / np.outer(s, s)
    gh = g[free] / s
    out.update(s=s, C=C, gh=gh)
    A = C + lam * np.eye(free.size)
    try:
        Lc = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        out["ok"] = False
        return out
    y = np.linalg.solve(Lc.T, np.linalg.solve(Lc, gh))
    if not np.all(np.isfinite(y)):
        out["ok"] = False
        return out
    trial = theta.copy()
    trial[free] = np.clip(theta[free] + y / s, lb[free], ub[free])
    out.update(y=y, theta_trial=trial, pred=float(gh @ y - 0.5 * y @ (C @ y)))
    return out


def step(F, g, theta, lb, ub, lam, freeze_tol=1e-6):
    r = step_full(F, g, theta, lb, ub, lam, freeze_tol)
    return r["theta_trial"], r["pred"], r["held"]


def evaluate(theta, lb, ub, instruments):
    """(lnprob, F, g) of one row by the yardsticks."""
    lp = vo.lnprob(theta, lb, ub, instruments)
    if not np.isfinite(lp):
        return lp, None, None
    return lp, fr.fisher(theta, instruments)[0], gr.lnlike_grad(theta, instruments)[1]


def nielsen_accept(lam, rho):
    return lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3)


def accept(lam, nu, lp, lt, pred, ynorm, ok, ftol, xtol, lambda_max):
    """The accept rule of one iteration of one row, as ``lm_accept_kernel`` states it -> (accepted, lam, nu, status).
    lp, lt: lnprob at theta and at the trial point; pred, ynorm (|y|_inf; 0 when every index is held), ok: the solve's."""
    accepted, status = False, 0
    if ok:
        if np.isfinite(lt) and lt > lp:
            gain = lt - lp
            accepted = True
            if gain <= ftol * max(1.0, abs(lp)):
                status = 1
            lam, nu = nielsen_accept(lam, gain / pred), 2.0
        if ynorm <= xtol:
            status = 1
    if not accepted:
        lam, nu = lam * nu, 2.0 * nu
    if status == 0 and lam > lambda_max:
        status = 3
    return accepted, lam, nu, status


def ynorm_estimate(trial, theta, F, held, lb, ub, xtol):
    """|y|_inf read off a solve's outputs, for callers that are not given it (vp_lm_solve returns none) -> (estimate, determined).
    The estimate is max |trial_k - theta_k| sqrt(F_kk) over the free indices the clip did not touch; it is exact (0) when every
    index is held.  ``determined`` is False where the estimate cannot say on which side of xtol |y|_inf lies: within a factor 2 of
    xtol, or at most 2 xtol with a clipped index (whose y_k is unknown).  With xtol = 0 every pair is determined: |y|_inf = 0 with a
    free index needs gh = 0 to the bit, and the estimate is then reported as the smallest positive double at least."""
    free = ~held
    if not np.any(free):
        return 0.0, True
    clipped = free & ((trial == lb) | (trial == ub))
    use = free & ~clipped
    est = float(np.max(np.abs(trial - theta)[use] * np.sqrt(np.diag(F)[use]))) if np.any(use) else 0.0
    if xtol == 0.0:
        return max(est, np.finfo(np.float64).tiny), True
    if 0.5 * xtol <= est <= 2.0 * xtol or (np.any(clipped) and est <= 2.0 * xtol):
        return est, False
    return est, True


def run(theta0, lb, ub, instruments, nsteps=50, lambda0=1e-3, lambda_max=1e12, ftol=1e-10, xtol=1e-6, freeze_tol=1e-6, trace=None):
    """``trace``: a list that receives one dict per iteration (the inputs and outputs of ``accept`` and of the solve)."""
    theta = np.array(theta0, dtype=np.float64)
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    lp, F, g = evaluate(theta, lb, ub, instruments)
    if not np.isfinite(lp):
        return dict(theta=theta, lnprob=np.nan, status=2, niter=0, naccept=0, lam=np.nan, history=[], F=None, g=None, held=None)
    lam, nu, status, niter, nacc = float(lambda0), 2.0, 0, 0, 0
    history = [lp]
    held = held_set(F, g, theta, lb, ub, freeze_tol)
    while status == 0 and niter < nsteps:
        niter += 1
        r = step_full(F, g, theta, lb, ub, lam, freeze_tol)
        held = r["held"]
        lt = vo.lnprob(r["theta_trial"], lb, ub, instruments) if r["ok"] else np.nan
        ynorm = float(np.max(np.abs(r["y"]))) if r["y"].size else 0.0
        rec = dict(lam=lam, nu=nu, lp=lp, lt=lt, pred=r["pred"], ynorm=ynorm, ok=r["ok"], theta=theta, trial=r["theta_trial"], held=held, F=F)
        accepted, lam, nu, status = accept(lam, nu, lp, lt, r["pred"], ynorm, r["ok"], ftol, xtol, lambda_max)
        if trace is not None:
            rec.update(accepted=accepted, lam_out=lam, status=status)
            trace.append(rec)
        if accepted:
            theta, lp = r["theta_trial"], lt
            nacc += 1
            history.append(lp)
            if status == 0:
                _, F, g = evaluate(theta, lb, ub, instruments)
    if nacc and (status != 0 or niter >= nsteps):
        _, F, g = evaluate(theta, lb, ub, instruments)
    return dict(theta=theta, lnprob=lp, status=status, niter=niter, naccept=nacc, lam=lam, history=history, F=F, g=g, held=held)


def stationarity(F, g, theta, lb, ub, freeze_tol=1e-6):
    """max_k |g_k| / sqrt(F_kk) over the free set (0 when every index is held)."""
    held = held_set(F, g, theta, lb, ub, freeze_tol)
    if np.all(held):
        return 0.0
    return float(np.max(np.abs(g[~held]) / np.sqrt(np.diag(F)[~held])))
