// capi_grad.inc -- entry points: lnprob with its analytic gradient (grad_kernels.h), the test hooks for w(z) and its derivatives.
// A fragment of the ONE translation unit capi.hip (included there inside extern "C", in order; not a header of its own).
namespace {

// What the gradient path does not take (refused with VP_EINVAL, never a fallback).
int grad_refusals(vp_ctx* c, const char* entry = "vp_lnprob_grad_batch", const char* what = "analytic gradient") {
    for (size_t k = 0; k < c->inst.size(); ++k) {
        const Instrument& in = c->inst[k];
        if (in.dev.method != VP_VOIGT_WOFZ)
            return fail(c, VP_EINVAL, std::string(entry) + ": instrument " + std::to_string(k) +
                        " uses voigt_method 'fast' (piecewise formula): no " + what);
        if (in.nanfix)
            return fail(c, VP_EINVAL, std::string(entry) + ": instrument " + std::to_string(k) +
                        " has NaN wavelength samples: no " + what);
    }
    return VP_OK;
}

int grad_grow(vp_ctx* c, double** p, size_t* have, size_t need) {
    if (need <= *have) return VP_OK;
    HIP_TRY(c, hipDeviceSynchronize());          // a stream-ordered previous call may still be using the old buffer
    if (*p) HIP_TRY(c, hipFree(*p));
    *p = nullptr; *have = 0;
    HIP_TRY(c, hipMalloc((void**)p, need * sizeof(double)));
    *have = need;
    return VP_OK;
}

// Rows per pass: the (rows, P) buffers stay below 2^25 doubles each, and a grid's z extent below 2^15.
int grad_rows_per_pass(const vp_ctx* c, int W) {
    int Pmax = 1;
    for (auto& in : c->inst) Pmax = std::max(Pmax, in.dev.P);
    return std::max(1, std::min({W, 32768, (1 << 25) / Pmax}));
}

// the workspace of a W-row gradient batch
int grad_grow_batch(vp_ctx* c, int W) {
    int rc;
    if ((rc = ensure_workspace(c, W))) return rc;
    const int Wc = grad_rows_per_pass(c, W);
    size_t n_px = 0, n_rec = 0, n_part = 0;
    for (auto& in : c->inst) {
        const size_t nchunk = (in.dev.P + vp::GRAD_CHUNK - 1) / vp::GRAD_CHUNK;
        n_px = std::max(n_px, (size_t)Wc * in.dev.P);
        n_rec = std::max(n_rec, (size_t)Wc * in.dev.L * vp::LC_STRIDE);
        n_part = std::max(n_part, (size_t)Wc * in.dev.L * nchunk * 3);
    }
    auto& G = c->grad;
    if ((rc = grad_grow(c, &G.fl, &G.n_fl, n_px)) || (rc = grad_grow(c, &G.q, &G.n_q, n_px)) ||
        (rc = grad_grow(c, &G.rec, &G.n_rec, n_rec)) || (rc = grad_grow(c, &G.part, &G.n_part, n_part)))
        return rc;
    return VP_OK;
}

// (called with c->mu held) the adjoint launches for the rows whose d_lnprob entry is finite (the others get NaN rows), on `s`
int enqueue_grad_rows(vp_ctx* c, int W, const double* d_theta, const double* d_lnprob, double* d_grad, hipStream_t s) {
    int rc;
    if ((rc = grad_grow_batch(c, W))) return rc;
    const int D = c->D, Wc = grad_rows_per_pass(c, W), T = vp::GRAD_THREADS;
    auto& G = c->grad;
    hipLaunchKernelGGL(vp::grad_init_kernel, dim3((unsigned)(((size_t)W * D + T - 1) / T)), dim3(T), 0, s, d_lnprob, W, D, d_grad);
    for (auto& in : c->inst) {
        const vp::InstDev& I = in.dev;
        vp::LinesDev L = in.lines;
        L.NCm = 0;                                        // line records only
        const int nchunk = (I.P + vp::GRAD_CHUNK - 1) / vp::GRAD_CHUNK;
        for (int w0 = 0; w0 < W; w0 += Wc) {
            const int n = std::min(Wc, W - w0);
            // the workspace was sized above from the same quantities; checked here all the same, launch by launch
            if ((size_t)n * I.P > G.n_fl || (size_t)n * I.P > G.n_q || (size_t)n * I.L * vp::LC_STRIDE > G.n_rec ||
                (size_t)n * I.L * nchunk * 3 > G.n_part || I.L != L.L)
                return fail(c, VP_ESTATE, "vp_lnprob_grad_batch: workspace smaller than the launch needs");
            const double* th = d_theta + (size_t)w0 * D;
            const double* lp = d_lnprob + w0;
            const dim3 gpx((I.P + T - 1) / T, n);
            hipLaunchKernelGGL(vp::grad_prep_kernel, dim3((unsigned)(((size_t)n * I.L + 63) / 64)), dim3(64), 0, s, th, lp, n, D, L, G.rec);
            hipLaunchKernelGGL(vp::grad_flux_kernel, gpx, dim3(T), 0, s, I, G.rec, lp, G.fl);
            hipLaunchKernelGGL(vp::grad_q_kernel, gpx, dim3(T), 0, s, I, lp, G.fl, G.q);
            hipLaunchKernelGGL(vp::grad_s_kernel, gpx, dim3(T), 0, s, I, lp, G.q, G.fl);
            hipLaunchKernelGGL(vp::grad_lines_kernel, dim3(nchunk, I.L, n), dim3(T), 0, s, I, G.rec, lp, G.fl, G.part, nchunk);
            hipLaunchKernelGGL(vp::grad_reduce_kernel, dim3((unsigned)(((size_t)n * D + T - 1) / T)), dim3(T), 0, s, L, lp, G.part, nchunk, n, D,
                               d_grad + (size_t)w0 * D);
        }
    }
    HIP_TRY(c, hipGetLastError());
    return VP_OK;
}

// (called with c->mu held) lnprob by the value path's own launches, then the adjoint launches, all on `s`
int enqueue_lnprob_grad(vp_ctx* c, int W, const double* d_theta, double* d_lnprob, double* d_grad, hipStream_t s) {
    int rc;
    if ((rc = grad_grow_batch(c, W)) || (rc = enqueue_lnprob(c, W, d_theta, d_lnprob, s))) return rc;
    return enqueue_grad_rows(c, W, d_theta, d_lnprob, d_grad, s);
}

}  // namespace

int vp_lnprob_grad_batch_device(vp_ctx* c, int W, int D, const double* d_theta, double* d_lnprob, double* d_grad, void* hip_stream) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    int rc = check_batch_args(c, W, D, d_theta, d_lnprob);
    if (rc) return rc;
    if (W > 0 && !d_grad) return fail(c, VP_EINVAL, "NULL grad");
    if ((rc = grad_refusals(c))) return rc;
    if (W == 0) return VP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if ((rc = foreign_stream_fence(c, s))) return rc;
    return enqueue_lnprob_grad(c, W, d_theta, d_lnprob, d_grad, s);
}

int vp_lnprob_grad_batch(vp_ctx* c, int W, int D, const double* theta, double* lnprob, double* grad) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    int rc = check_batch_args(c, W, D, theta, lnprob);
    if (rc) return rc;
    if (W > 0 && !grad) return fail(c, VP_EINVAL, "NULL grad");
    if ((rc = grad_refusals(c))) return rc;
    if (W == 0) return VP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    auto& G = c->grad;
    const size_t nt = (size_t)W * D;
    if ((rc = grad_grow(c, &G.io, &G.n_io, 2 * nt + W))) return rc;
    double* d_theta = G.io;
    double* d_grad = G.io + nt;
    double* d_lnprob = G.io + 2 * nt;
    HIP_TRY(c, hipMemcpyAsync(d_theta, theta, nt * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = enqueue_lnprob_grad(c, W, d_theta, d_lnprob, d_grad, c->stream))) return rc;
    HIP_TRY(c, hipMemcpyAsync(grad, d_grad, nt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(lnprob, d_lnprob, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return VP_OK;
}

int vp_voigt_w(vp_ctx* c, int na, const double* a, int nx, const double* x, double* H, double* L) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    if (na <= 0 || nx <= 0 || !a || !x || !H || !L) return fail(c, VP_EINVAL, "vp_voigt_w: empty or NULL input");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t no = (size_t)na * nx;
    int rc;
    if ((rc = ensure_scratch(c, (na + nx + 2 * no) * sizeof(double)))) return rc;
    double* d_a = c->d_scratch;
    double* d_x = d_a + na;
    double* d_H = d_x + nx;
    double* d_L = d_H + no;
    HIP_TRY(c, hipMemcpyAsync(d_a, a, na * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_x, x, nx * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(vp::voigt_w_kernel, dim3((nx + vp::GRAD_THREADS - 1) / vp::GRAD_THREADS, na), dim3(vp::GRAD_THREADS), 0, c->stream,
                       d_a, d_x, nx, d_H, d_L);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(H, d_H, no * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(L, d_L, no * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return VP_OK;
}

int vp_voigt_dw(vp_ctx* c, int na, const double* a, int nx, const double* x, double* H, double* Hx, double* G) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    if (na <= 0 || nx <= 0 || !a || !x || !H || !Hx || !G) return fail(c, VP_EINVAL, "vp_voigt_dw: empty or NULL input");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t no = (size_t)na * nx;
    int rc;
    if ((rc = ensure_scratch(c, (na + nx + 3 * no) * sizeof(double)))) return rc;
    double* d_a = c->d_scratch;
    double* d_x = d_a + na;
    double* d_H = d_x + nx;
    double* d_Hx = d_H + no;
    double* d_G = d_Hx + no;
    HIP_TRY(c, hipMemcpyAsync(d_a, a, na * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_x, x, nx * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(vp::voigt_dw_kernel, dim3((nx + vp::GRAD_THREADS - 1) / vp::GRAD_THREADS, na), dim3(vp::GRAD_THREADS), 0, c->stream,
                       d_a, d_x, nx, d_H, d_Hx, d_G);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(H, d_H, no * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(Hx, d_Hx, no * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(G, d_G, no * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return VP_OK;
}
