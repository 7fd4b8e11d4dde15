"""Times the analytic gradient against what it replaces, device resident, one process:
  (a) vp_lnprob_grad_batch_device on W rows,
  (b) the finite-difference stencil the host builds today: vp_lnprob_batch_device on W (D+1) rows,
  (c) plain vp_lnprob_batch_device on W rows,
for C1, C2, C3 at their BASELINE walker counts.  Warm-up, then `--reps` repetitions each timed with HIP events on the
context's stream; medians.  Prints one JSON line per config.  `--only c` runs (c) alone (a build without the gradient)."""
import argparse
import json
import sys
import os

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C1,C2,C3")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="abc")
    args = ap.parse_args()
    import torch
    from rbvfit_amd.workloads import make_workload
    dev = torch.device("cuda", 0)
    for name in args.configs.split(","):
        wl = make_workload(name)
        eng, W, D = wl.engine, len(wl.thetas), wl.ndim
        stream = torch.cuda.ExternalStream(eng.stream_handle, device=dev)
        th = torch.as_tensor(np.ascontiguousarray(wl.thetas), device=dev)
        eps = 1e-8
        stencil = np.repeat(wl.thetas[:, None, :], D + 1, axis=1)
        for k in range(D):
            stencil[:, k + 1, k] += np.where(wl.thetas[:, k] + eps > wl.ub[k], -eps, eps)
        st = torch.as_tensor(np.ascontiguousarray(stencil.reshape(-1, D)), device=dev)
        lp = torch.empty(W, dtype=torch.float64, device=dev)
        lps = torch.empty(W * (D + 1), dtype=torch.float64, device=dev)
        g = torch.empty((W, D), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        runs = {"c": lambda: eng.lnprob_device(th.data_ptr(), lp.data_ptr(), W, 0),
                "b": lambda: eng.lnprob_device(st.data_ptr(), lps.data_ptr(), W * (D + 1), 0)}
        if "a" in args.only:
            runs["a"] = lambda: eng.lnprob_grad_device(th.data_ptr(), lp.data_ptr(), g.data_ptr(), W, 0)
        out = {"config": name, "W": W, "D": D, "reps": args.reps}
        for key in sorted(k for k in runs if k in args.only):
            ts = []
            for i in range(args.warmup + args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                runs[key]()
                e1.record(stream)
                e1.synchronize()
                if i >= args.warmup:
                    ts.append(e0.elapsed_time(e1) * 1e3)
            out["%s_us_median" % key] = float(np.median(ts))
            out["%s_us_min" % key] = float(np.min(ts))
        if "a_us_median" in out:
            out["b_over_a"] = out["b_us_median"] / out["a_us_median"] if "b_us_median" in out else None
            out["a_over_c"] = out["a_us_median"] / out["c_us_median"] if "c_us_median" in out else None
        print(json.dumps(out), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
