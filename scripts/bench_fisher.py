"""Times one Engine.fisher call (host entry: theta in, lnprob and (W, D, D) out) against the route open without it, on the same
build, for C1, C2, C3 at W = 1 and W = 64:
  (a) Engine.fisher on W rows,
  (b) the stencil route: Engine.model_flux on the 2D+1 central-stencil rows of every theta and instrument (h_k = 1e-5 max(1, |theta_k|)),
      the Jacobian by differences on the host, J^T W J in NumPy -- (2D+1) P doubles per theta and instrument cross PCIe,
  (c) plain Engine.lnprob and (d) Engine.lnprob_grad on the same rows, for the unchanged paths.
Warm-up, then `--reps` repetitions each, wall clock around the blocking call; medians.  Prints one JSON line per (config, W),
with the worst |F_a - F_b| / sqrt(F_jj F_kk) as a sanity figure (the stencil's truncation error, not a test)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stencil_fisher(eng, spectra, rows):
    W, D = rows.shape
    h = 1e-5 * np.maximum(1.0, np.abs(rows))
    st = np.repeat(rows[:, None, :], 2 * D + 1, axis=1)
    for k in range(D):
        st[:, 1 + k, k] += h[:, k]
        st[:, 1 + D + k, k] -= h[:, k]
    F = np.zeros((W, D, D))
    for i, (_, _, err) in enumerate(spectra):
        m = eng.model_flux(i, st.reshape(-1, D)).reshape(W, 2 * D + 1, -1)
        J = (m[:, 1:D + 1] - m[:, D + 1:]) / (2 * h[:, :, None])
        F += np.einsum("wjp,wkp->wjk", J / np.asarray(err, dtype=np.float64) ** 2, J)
    return F


def timed(fn, warmup, reps):
    ts = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if i >= warmup:
            ts.append((t1 - t0) * 1e6)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1,C2,C3")
    ap.add_argument("--walkers", default="1,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="abcd")
    args = ap.parse_args()
    from rbvfit_amd.workloads import make_workload
    for name in args.configs.split(","):
        wl = make_workload(name)
        eng, D = wl.engine, wl.ndim
        for W in (int(w) for w in args.walkers.split(",")):
            rows = np.ascontiguousarray(np.vstack([wl.theta_true[None, :], wl.thetas])[:W])
            out = {"config": name, "W": W, "D": D, "pixels": list(wl.pixels), "reps": args.reps}
            runs = {"a": lambda: eng.fisher(rows), "b": lambda: stencil_fisher(eng, wl.spectra, rows),
                    "c": lambda: eng.lnprob(rows), "d": lambda: eng.lnprob_grad(rows)}
            for key in sorted(k for k in runs if k in args.only):
                out["%s_us_median" % key], out["%s_us_min" % key] = timed(runs[key], args.warmup, args.reps)
            if "a" in args.only and "b" in args.only:
                lp, Fa = eng.fisher(rows)
                Fb = stencil_fisher(eng, wl.spectra, rows)
                fin = np.isfinite(lp)
                if np.any(fin):
                    d = np.sqrt(np.einsum("wjj->wj", Fa[fin]))
                    with np.errstate(divide="ignore", invalid="ignore"):
                        out["stencil_vs_analytic"] = float(np.nanmax(np.abs(Fa[fin] - Fb[fin]) / (d[:, :, None] * d[:, None, :])))
                out["finite_rows"] = int(fin.sum())
                out["b_over_a"] = out["b_us_median"] / out["a_us_median"]
            print(json.dumps(out), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
