"""Times the batched Levenberg-Marquardt fit (Engine.lm_run / vfit.fit_lm) on C1 and C2 at W = 1, 16, 64 starts, against what the
same build offers without it:
  (a) Engine.lm_run: wall time of `--nsteps` iterations minus that of nsteps = 0, per iteration the slowest row took part in;
  (b) the same iteration assembled on the host from the entry points this work leaves unchanged: Engine.fisher +
      Engine.lnprob_grad + one scaled, damped np.linalg.solve per row + Engine.lnprob on the trial rows -- theta, F and g cross
      PCIe every iteration;
  (c) the parts of (b) one by one (where an iteration's time goes);
  (d) vfit.fit_lm(starts) against W serial vfit.fit_quick(grad="analytic") calls from the same starts, with the best lnprob of each.
Starts: the workload's truth plus `--spread` of the box width, uniform, row 0 the truth's neighbour the workload itself makes.
Warm-up, then `--reps` repetitions, wall clock around the blocking call; medians.  One JSON line per (config, W), printed and
appended to `--out` (default profiles/lm_bench.jsonl; "" for none).
`--trace CONFIG,W` runs only (a) a few times, for a kernel trace taken from outside."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup, reps):
    ts = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if i >= warmup:
            ts.append((t1 - t0) * 1e6)
    return float(np.median(ts))


def host_iteration(eng, rows, lb, ub, lam=1e-3, freeze_tol=1e-6):
    lp, F = eng.fisher(rows)
    _, g = eng.lnprob_grad(rows)
    trial = rows.copy()
    for w in range(len(rows)):
        d = np.diag(F[w])
        held = ((rows[w] == lb) & (g[w] < 0)) | ((rows[w] == ub) & (g[w] > 0)) | ~(d > 0) | (d * (ub - lb) ** 2 < freeze_tol)
        fr = np.nonzero(~held)[0]
        if fr.size == 0 or not np.isfinite(lp[w]):
            continue
        s = np.sqrt(d[fr])
        y = np.linalg.solve(F[w][np.ix_(fr, fr)] / np.outer(s, s) + lam * np.eye(fr.size), g[w][fr] / s)
        trial[w, fr] = np.clip(rows[w, fr] + y / s, lb[fr], ub[fr])
    return eng.lnprob(trial)


def starts_of(wl, W, spread, seed=5):
    rng = np.random.default_rng(seed)
    st = wl.theta_true[None, :] + spread * (wl.ub - wl.lb)[None, :] * rng.uniform(-1, 1, (W, wl.ndim))
    st[0] = wl.thetas[0]
    return np.ascontiguousarray(np.clip(st, wl.lb, wl.ub))


def fitter_of(wl, theta):
    from rbvfit_amd import vfit as mc
    data = {"I%d" % i: {"model": t, "wave": w, "flux": f, "error": e} for i, (t, (w, f, e)) in enumerate(zip(wl.tables, wl.spectra))}
    return mc.vfit(data, theta, wl.lb, wl.ub, no_of_Chain=16, no_of_steps=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1,C2")
    ap.add_argument("--walkers", default="1,16,64")
    ap.add_argument("--nsteps", type=int, default=8)
    ap.add_argument("--spread", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="abcd")
    ap.add_argument("--trace", default="")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lm_bench.jsonl"))
    args = ap.parse_args()
    from rbvfit_amd.workloads import make_workload
    if args.trace:
        name, W = args.trace.split(",")
        wl = make_workload(name)
        rows = starts_of(wl, int(W), args.spread)
        for _ in range(3):
            res = wl.engine.lm_run(rows, nsteps=args.nsteps)
        print(json.dumps({"config": name, "W": int(W), "niter": res.niter.tolist(), "status": res.status.tolist()}))
        wl.engine.close()
        return
    for name in args.configs.split(","):
        wl = make_workload(name)
        eng, D = wl.engine, wl.ndim
        for W in (int(w) for w in args.walkers.split(",")):
            rows = starts_of(wl, W, args.spread)
            out = {"config": name, "W": W, "D": D, "pixels": list(wl.pixels), "nsteps": args.nsteps, "spread": args.spread, "reps": args.reps}
            if "a" in args.only:
                res = eng.lm_run(rows, nsteps=args.nsteps)
                t0 = timed(lambda: eng.lm_run(rows, nsteps=0), args.warmup, args.reps)
                tn = timed(lambda: eng.lm_run(rows, nsteps=args.nsteps), args.warmup, args.reps)
                its = int(res.niter.max())
                out.update(lm_run_0_us=t0, lm_run_n_us=tn, lm_iterations=its, lm_niter_mean=float(res.niter.mean()),
                           lm_status=np.bincount(res.status, minlength=4).tolist(), lm_us_per_iteration=(tn - t0) / max(its, 1))
            if "b" in args.only:
                out["host_us_per_iteration"] = timed(lambda: host_iteration(eng, rows, wl.lb, wl.ub), args.warmup, args.reps)
            if "c" in args.only:
                out["fisher_us"] = timed(lambda: eng.fisher(rows), args.warmup, args.reps)
                out["lnprob_grad_us"] = timed(lambda: eng.lnprob_grad(rows), args.warmup, args.reps)
                out["lnprob_us"] = timed(lambda: eng.lnprob(rows), args.warmup, args.reps)
            if "a" in args.only and "b" in args.only:
                out["host_over_lm"] = out["host_us_per_iteration"] / out["lm_us_per_iteration"]
            if "d" in args.only:
                fit = fitter_of(wl, rows[0])
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    fit.fit_lm(starts=rows)
                    t0 = time.perf_counter()
                    fit.fit_lm(starts=rows)
                    t1 = time.perf_counter()
                    best_q = -np.inf
                    for t in rows:
                        fit.theta = t
                        q, _ = fit.fit_quick(grad="analytic")
                        best_q = max(best_q, float(fit.lnprob(q)))
                    t2 = time.perf_counter()
                r = fit.lm_result
                out.update(fit_lm_ms=(t1 - t0) * 1e3, fit_quick_serial_ms=(t2 - t1) * 1e3, fit_lm_best_lnprob=float(r.lnprob[r.best()]),
                           fit_quick_best_lnprob=best_q, fit_lm_status=np.bincount(r.status, minlength=4).tolist(),
                           fit_lm_niter_max=int(r.niter.max()))
                fit.close()
            print(json.dumps(out), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(out) + "\n")
        eng.close()


if __name__ == "__main__":
    main()
