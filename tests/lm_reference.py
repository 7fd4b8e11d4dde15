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
0 running / out of iterations, 1 converged, 2 start not evaluable, 3 stalled (lam > lambda_max).
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


def run(theta0, lb, ub, instruments, nsteps=50, lambda0=1e-3, lambda_max=1e12, ftol=1e-10, xtol=1e-6, freeze_tol=1e-6):
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
        accepted = False
        if r["ok"]:
            lt = vo.lnprob(r["theta_trial"], lb, ub, instruments)
            if np.isfinite(lt) and lt > lp:
                gain = lt - lp
                accepted = True
                if gain <= ftol * max(1.0, abs(lp)):
                    status = 1
                lam, nu = nielsen_accept(lam, gain / r["pred"]), 2.0
                theta, lp = r["theta_trial"], lt
                nacc += 1
                history.append(lp)
            if r["y"].size == 0 or np.max(np.abs(r["y"])) <= xtol:
                status = 1
        if not accepted:
            lam, nu = lam * nu, 2.0 * nu
        if status == 0 and lam > lambda_max:
            status = 3
        if accepted and status == 0:
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
