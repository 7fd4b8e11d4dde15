// capi_lm.inc -- entry points: the batched Levenberg-Marquardt fit (vp_lm_run) and the test hook on its solve (vp_lm_solve), lm_kernels.h.
// A fragment of the ONE translation unit capi.hip (included there inside extern "C", in order; not a header of its own).
namespace {

int lm_check_D(vp_ctx* c, const char* entry, int D) {
    if (D > vp::LM_MAX_D)
        return fail(c, VP_EINVAL, std::string(entry) + ": D=" + std::to_string(D) + " parameters; the solve keeps a row's packed triangle in LDS and "
                    "takes at most " + std::to_string(vp::LM_MAX_D));
    if (vp::lm_step_lds_bytes(D) > c->lds_limit) return fail(c, VP_ESTATE, std::string(entry) + ": the packed triangle does not fit the device's LDS");
    return VP_OK;
}

// one workgroup per row, one lane per theta index: a wave where D <= 64, two above
void launch_lm_step(int W, int D, const vp::LmStep& a, hipStream_t s) {
    hipLaunchKernelGGL(vp::lm_step_kernel, dim3(W), dim3(D <= 64 ? 64 : 128), vp::lm_step_lds_bytes(D), s, a, D);
}

}  // namespace

int vp_lm_solve(vp_ctx* c, int W, int D, const double* F, const double* g, const double* theta, const double* lambda,
                double* theta_trial, double* pred, int* held, int* ok) {
    if (!c) return VP_EINVAL;
    CtxGuard guard(c);
    if (c->D <= 0) return fail(c, VP_ESTATE, "vp_set_bounds has not been called");
    if (D != c->D) return fail(c, VP_EINVAL, "theta has D=" + std::to_string(D) + " but the context was set up with D=" + std::to_string(c->D));
    if (W < 0) return fail(c, VP_EINVAL, "negative batch size");
    if (W > 0 && (!F || !g || !theta || !lambda || !theta_trial || !pred || !held || !ok)) return fail(c, VP_EINVAL, "vp_lm_solve: NULL argument");
    int rc;
    if ((rc = lm_check_D(c, "vp_lm_solve", D))) return rc;
    if (W == 0) return VP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nt = (size_t)W * D, nf = nt * D;
    struct Dev { double *F, *g, *theta, *lam, *trial, *pred, *ynorm; int *held, *ok; } d;
    if ((rc = carve_scratch(c, [&](Arena& A) {
        d.F = A.take<double>(nf); d.g = A.take<double>(nt); d.theta = A.take<double>(nt); d.lam = A.take<double>(W);
        d.trial = A.take<double>(nt); d.pred = A.take<double>(W); d.ynorm = A.take<double>(W);
        d.held = A.take<int>(nt); d.ok = A.take<int>(W);
    }))) return rc;
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemcpyAsync(d.F, F, nf * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d.g, g, nt * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d.theta, theta, nt * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d.lam, lambda, (size_t)W * sizeof(double), hipMemcpyHostToDevice, s));
    vp::LmStep a{d.F, d.g, d.theta, c->d_lb, c->d_ub, d.lam, nullptr, 1e-6, d.trial, d.pred, d.ynorm, d.held, d.ok};
    launch_lm_step(W, D, a, s);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(theta_trial, d.trial, nt * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(pred, d.pred, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(held, d.held, nt * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(ok, d.ok, (size_t)W * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return VP_OK;
}

int vp_lm_run(vp_ctx* c, int W, int D, double* theta, double* lnprob, double* fisher, int* status, int* niter, double* lambda_out,
              int nsteps, const double* opts) {
    if (!c) return VP_EINVAL;
    CtxGuard guard(c);
    int rc = check_batch_args(c, W, D, theta, lnprob);
    if (rc) return rc;
    if (W > 0 && (!status || !niter || !lambda_out)) return fail(c, VP_EINVAL, "vp_lm_run: NULL status / niter / lambda_out");
    if ((rc = grad_refusals(c, "vp_lm_run", "Levenberg-Marquardt fit"))) return rc;
    const double lambda0 = opts ? opts[0] : 1e-3, lambda_max = opts ? opts[1] : 1e12, ftol = opts ? opts[2] : 1e-10,
                 xtol = opts ? opts[3] : 1e-6, freeze_tol = opts ? opts[4] : 1e-6;
    if (nsteps < 0 || !(lambda0 > 0.0) || !(lambda_max >= lambda0) || !(ftol >= 0.0) || !(xtol >= 0.0) || !(freeze_tol >= 0.0))
        return fail(c, VP_EINVAL, "vp_lm_run: nsteps >= 0, 0 < lambda0 <= lambda_max, ftol >= 0, xtol >= 0 and freeze_tol >= 0 required");
    if ((rc = lm_check_D(c, "vp_lm_run", D))) return rc;
    if (W == 0) return VP_OK;
    if ((size_t)W * D * D > 0x7fffffffu) return fail(c, VP_EINVAL, "vp_lm_run: W x D x D does not fit an int");
    HIP_TRY(c, hipSetDevice(c->device));
    // the workspaces of the three reused paths first: growing one synchronises the device and must not happen inside the loop
    if ((rc = fisher_grow(c, W)) || (rc = grad_grow_batch(c, W))) return rc;
    const size_t nt = (size_t)W * D, nf = nt * D;
    struct Dev { vp::LmState S; double *F, *g, *Ft, *gt, *mask, *trial, *lpt, *pred, *ynorm; int* ok; } d;
    if ((rc = carve_scratch(c, [&](Arena& A) {
        d.S.theta = A.take<double>(nt); d.S.lp = A.take<double>(W); d.S.lam = A.take<double>(W); d.S.nu = A.take<double>(W);
        d.F = A.take<double>(nf); d.g = A.take<double>(nt); d.Ft = A.take<double>(nf); d.gt = A.take<double>(nt);
        d.mask = A.take<double>(W); d.trial = A.take<double>(nt); d.lpt = A.take<double>(W); d.pred = A.take<double>(W);
        d.ynorm = A.take<double>(W);
        d.S.status = A.take<int>(W); d.S.niter = A.take<int>(W); d.S.nacc = A.take<int>(W); d.S.stale = A.take<int>(W);
        d.S.running = A.take<int>(16); d.ok = A.take<int>(W);
    }))) return rc;
    hipStream_t s = c->stream;
    const int T = vp::LM_THREADS;
    const dim3 grow((W + T - 1) / T), gkeep((unsigned)(((size_t)W * ((size_t)D * D + D) + T - 1) / T));
    int h_running = 0;
    // (whatever way this call ends -- an error return from the middle of the loop included -- nothing of it is left running on the
    //  stream, reading this call's scratch or the caller's theta or writing h_running, when the context's mutex is released)
    struct Drain { hipStream_t q; ~Drain() { (void)hipStreamSynchronize(q); } } drain{s};
    HIP_TRY(c, hipMemcpyAsync(d.S.theta, theta, nt * sizeof(double), hipMemcpyHostToDevice, s));
    if ((rc = enqueue_lnprob(c, W, d.S.theta, d.S.lp, s))) return rc;
    hipLaunchKernelGGL(vp::lm_init_kernel, dim3(1), dim3(T), 0, s, W, d.S, lambda0);
    // F and g of the rows that moved (every evaluable row at first): the Fisher and gradient launches skip the rows the mask leaves NaN
    auto evaluate = [&](bool need_running, bool with_grad) -> int {
        int r;
        hipLaunchKernelGGL(vp::lm_mask_kernel, grow, dim3(T), 0, s, W, d.S, need_running ? 1 : 0, d.mask);
        if ((r = enqueue_fisher_rows(c, W, d.S.theta, d.mask, d.Ft, s))) return r;
        if (with_grad && (r = enqueue_grad_rows(c, W, d.S.theta, d.mask, d.gt, s))) return r;
        hipLaunchKernelGGL(vp::lm_keep_kernel, gkeep, dim3(T), 0, s, W, D, d.mask, d.Ft, with_grad ? d.gt : (const double*)nullptr, d.F, d.g, d.S.stale);
        return VP_OK;
    };
    HIP_TRY(c, hipMemcpyAsync(&h_running, d.S.running, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const vp::LmStep step{d.F, d.g, d.S.theta, c->d_lb, c->d_ub, d.S.lam, d.S.status, freeze_tol, d.trial, d.pred, d.ynorm, nullptr, d.ok};
    for (int it = 0; it < nsteps && h_running > 0; ++it) {
        if ((rc = evaluate(true, true))) return rc;
        launch_lm_step(W, D, step, s);
        if ((rc = enqueue_lnprob(c, W, d.trial, d.lpt, s))) return rc;
        hipLaunchKernelGGL(vp::lm_accept_kernel, dim3(1), dim3(T), 0, s, W, D, d.S, d.trial, d.lpt, d.pred, d.ynorm, d.ok, ftol, xtol, lambda_max);
        HIP_TRY(c, hipGetLastError());
        // the one word the host reads per iteration: rows still running
        HIP_TRY(c, hipMemcpyAsync(&h_running, d.S.running, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
    }
    if (fisher) {                                         // F at the result: the rows whose last trial was accepted
        if ((rc = evaluate(false, false))) return rc;
        HIP_TRY(c, hipMemcpyAsync(fisher, d.F, nf * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(theta, d.S.theta, nt * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(lnprob, d.S.lp, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(status, d.S.status, (size_t)W * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(niter, d.S.niter, (size_t)W * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(lambda_out, d.S.lam, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const double nan = std::nan("");
    for (int w = 0; w < W; ++w) {                         // a start that cannot be evaluated: theta as it came, everything else NaN
        if (status[w] != 2) continue;
        lnprob[w] = lambda_out[w] = nan;
        if (fisher) std::fill(fisher + (size_t)w * D * D, fisher + (size_t)(w + 1) * D * D, nan);
    }
    return VP_OK;
}
