// capi_fisher.inc -- entry points: the model Jacobian d model_flux / d theta and the Fisher matrix sum_inst J^T W J (fisher_kernels.h).
// A fragment of the ONE translation unit capi.hip (included there inside extern "C", in order; not a header of its own).
namespace {

// theta index -> (line, kind) terms of one instrument, by line then kind: made once, at the first call that needs it
int fisher_terms(vp_ctx* c, Instrument& in) {
    if (in.fisher_off) return VP_OK;
    const int L = in.dev.L, D = c->D;
    std::vector<int> off(D + 1, 0);
    std::vector<int2> terms;
    terms.reserve(3 * (size_t)L);
    for (int k = 0; k < D; ++k) {
        off[k] = (int)terms.size();
        for (int l = 0; l < L; ++l)
            for (int kind = 0; kind < 3; ++kind)
                if (in.h_idx[(size_t)kind * L + l] == k) terms.push_back(int2{l, kind});
    }
    off[D] = (int)terms.size();
    int rc;
    int2* d_terms = nullptr;
    if ((rc = upload<int2>(c, &in, terms.data(), terms.size(), &d_terms))) return rc;
    if ((rc = upload<int>(c, &in, off.data(), off.size(), &in.fisher_off))) return rc;
    in.fisher_terms = d_terms;
    return VP_OK;
}

int fisher_chunks(int P) { return (P + vp::FISHER_CHUNK - 1) / vp::FISHER_CHUNK; }

// Rows per pass: rows x D x P (the derivative rows) and rows x chunks x D x D (the partial blocks) stay below 2^25 doubles each,
// and a grid's z extent below 2^15.
int fisher_rows_per_pass(const vp_ctx* c, int W, bool blocks) {
    size_t per_row = 1;
    for (auto& in : c->inst) {
        per_row = std::max(per_row, (size_t)c->D * in.dev.P);
        if (blocks) per_row = std::max(per_row, (size_t)fisher_chunks(in.dev.P) * c->D * c->D);
    }
    return (int)std::max<size_t>(1, std::min<size_t>({(size_t)W, 32768, ((size_t)1 << 25) / per_row}));
}

// (called with c->mu held) the launches that leave d model_flux / d theta of rows [0, n) for one instrument in the workspace;
// *out points at the (n, D, P) result.  lp: a finite entry per row that is to be evaluated.
int enqueue_jacobian(vp_ctx* c, Instrument& in, int n, const double* th, const double* lp, bool convolved, hipStream_t s, const double** out) {
    int rc;
    if ((rc = fisher_terms(c, in))) return rc;
    const vp::InstDev& I = in.dev;
    vp::LinesDev L = in.lines;
    L.NCm = 0;                                            // line records only
    const int D = c->D, T = vp::GRAD_THREADS;
    auto& G = c->grad;
    auto& Fw = c->fisher;
    const bool conv = convolved && I.K > 1;
    // the callers size the workspace from the same quantities; checked here all the same, launch by launch
    if ((size_t)n * I.P > G.n_fl || (size_t)n * I.L * vp::LC_STRIDE > G.n_rec || (size_t)n * D * I.P > Fw.n_g ||
        (conv && (size_t)n * D * I.P > Fw.n_J) || I.L != L.L || n > 32768 || D > 65535)
        return fail(c, VP_ESTATE, "vp_fisher_batch: workspace smaller than the launch needs");
    hipLaunchKernelGGL(vp::grad_prep_kernel, dim3((unsigned)(((size_t)n * I.L + 63) / 64)), dim3(64), 0, s, th, lp, n, D, L, G.rec);
    hipLaunchKernelGGL(vp::grad_flux_kernel, dim3((I.P + T - 1) / T, n), dim3(T), 0, s, I, G.rec, lp, G.fl);
    hipLaunchKernelGGL(vp::fisher_rows_kernel, dim3((I.P + T - 1) / T, D, n), dim3(T), 0, s, I, G.rec, lp, G.fl, in.fisher_off, in.fisher_terms, D, Fw.g);
    *out = Fw.g;
    if (conv) {
        const size_t lds = (size_t)(vp::FISHER_CONV_TILE + I.K - 1) * sizeof(double);
        if (lds > c->lds_limit || I.K - 1 > vp::FISHER_CONV_TILE) return fail(c, VP_ESTATE, "vp_fisher_batch: LSF longer than the convolution tile's halo");
        hipLaunchKernelGGL(vp::fisher_conv_kernel, dim3((I.P + vp::FISHER_CONV_TILE - 1) / vp::FISHER_CONV_TILE, D, n), dim3(T), lds, s, I, lp, Fw.g, D, Fw.J);
        *out = Fw.J;
    }
    return VP_OK;
}

int fisher_grow_jacobian(vp_ctx* c, int Wc) {
    size_t n_px = 0, n_rec = 0, n_row = 0, n_conv = 0;
    for (auto& in : c->inst) {
        n_px = std::max(n_px, (size_t)Wc * in.dev.P);
        n_rec = std::max(n_rec, (size_t)Wc * in.dev.L * vp::LC_STRIDE);
        n_row = std::max(n_row, (size_t)Wc * c->D * in.dev.P);
        if (in.dev.K > 1) n_conv = std::max(n_conv, (size_t)Wc * c->D * in.dev.P);      // (no LSF: J is g)
    }
    int rc;
    auto& G = c->grad;
    auto& Fw = c->fisher;
    if ((rc = grad_grow(c, &G.fl, &G.n_fl, n_px)) || (rc = grad_grow(c, &G.rec, &G.n_rec, n_rec)) ||
        (rc = grad_grow(c, &Fw.g, &Fw.n_g, n_row)) || (rc = grad_grow(c, &Fw.J, &Fw.n_J, n_conv)))
        return rc;
    return VP_OK;
}

// the workspace of a W-row Fisher batch
int fisher_grow(vp_ctx* c, int W) {
    int rc;
    if ((rc = ensure_workspace(c, W))) return rc;
    const int D = c->D, Wc = fisher_rows_per_pass(c, W, true);
    if ((rc = fisher_grow_jacobian(c, Wc))) return rc;
    size_t n_part = 0;
    for (auto& in : c->inst) n_part = std::max(n_part, (size_t)Wc * fisher_chunks(in.dev.P) * D * D);
    auto& Fw = c->fisher;
    return grad_grow(c, &Fw.part, &Fw.n_part, n_part);
}

// (called with c->mu held) the Jacobian and Fisher launches for the rows whose d_lnprob entry is finite (the others get NaN blocks), on `s`
int enqueue_fisher_rows(vp_ctx* c, int W, const double* d_theta, const double* d_lnprob, double* d_fisher, hipStream_t s) {
    int rc;
    if ((rc = fisher_grow(c, W))) return rc;
    const int D = c->D, Wc = fisher_rows_per_pass(c, W, true), T = vp::GRAD_THREADS;
    auto& Fw = c->fisher;
    const size_t DD = (size_t)D * D;
    if (DD > 0x7fffffffu) return fail(c, VP_EINVAL, "vp_fisher_batch: D x D does not fit an int");
    hipLaunchKernelGGL(vp::grad_init_kernel, dim3((unsigned)(((size_t)W * DD + T - 1) / T)), dim3(T), 0, s, d_lnprob, W, (int)DD, d_fisher);
    const int nt = (D + vp::FISHER_TILE - 1) / vp::FISHER_TILE, npair = nt * (nt + 1) / 2;
    if (npair > 65535) return fail(c, VP_EINVAL, "vp_fisher_batch: more than 11552 parameters are not supported");
    for (auto& in : c->inst) {
        const vp::InstDev& I = in.dev;
        const int nchunk = fisher_chunks(I.P);
        for (int w0 = 0; w0 < W; w0 += Wc) {
            const int n = std::min(Wc, W - w0);
            const double* lp = d_lnprob + w0;
            const double* J = nullptr;
            if ((rc = enqueue_jacobian(c, in, n, d_theta + (size_t)w0 * D, lp, true, s, &J))) return rc;
            if ((size_t)n * nchunk * DD > Fw.n_part) return fail(c, VP_ESTATE, "vp_fisher_batch: workspace smaller than the launch needs");
            hipLaunchKernelGGL(vp::fisher_block_kernel, dim3(nchunk, npair, n), dim3(T), 0, s, I, lp, J, D, nchunk, Fw.part);
            hipLaunchKernelGGL(vp::fisher_reduce_kernel, dim3((unsigned)(((size_t)n * DD + T - 1) / T)), dim3(T), 0, s, lp, Fw.part, nchunk, n, D,
                               d_fisher + (size_t)w0 * DD);
        }
    }
    HIP_TRY(c, hipGetLastError());
    return VP_OK;
}

// (called with c->mu held) lnprob by the value path's own launches, then the Jacobian and Fisher launches, all on `s`
int enqueue_fisher(vp_ctx* c, int W, const double* d_theta, double* d_lnprob, double* d_fisher, hipStream_t s) {
    int rc;
    if ((rc = fisher_grow(c, W)) || (rc = enqueue_lnprob(c, W, d_theta, d_lnprob, s))) return rc;
    return enqueue_fisher_rows(c, W, d_theta, d_lnprob, d_fisher, s);
}

}  // namespace

int vp_fisher_batch_device(vp_ctx* c, int W, int D, const double* d_theta, double* d_lnprob, double* d_fisher, void* hip_stream) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    int rc = check_batch_args(c, W, D, d_theta, d_lnprob);
    if (rc) return rc;
    if (W > 0 && !d_fisher) return fail(c, VP_EINVAL, "NULL fisher");
    if ((rc = grad_refusals(c, "vp_fisher_batch", "Fisher matrix"))) return rc;
    if (W == 0) return VP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if ((rc = foreign_stream_fence(c, s))) return rc;
    return enqueue_fisher(c, W, d_theta, d_lnprob, d_fisher, s);
}

int vp_fisher_batch(vp_ctx* c, int W, int D, const double* theta, double* lnprob, double* fisher) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    int rc = check_batch_args(c, W, D, theta, lnprob);
    if (rc) return rc;
    if (W > 0 && !fisher) return fail(c, VP_EINVAL, "NULL fisher");
    if ((rc = grad_refusals(c, "vp_fisher_batch", "Fisher matrix"))) return rc;
    if (W == 0) return VP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    auto& Fw = c->fisher;
    const size_t nt = (size_t)W * D, nf = nt * D;
    if ((rc = grad_grow(c, &Fw.io, &Fw.n_io, nt + W + nf))) return rc;
    double* d_theta = Fw.io;
    double* d_lnprob = Fw.io + nt;
    double* d_fisher = Fw.io + nt + W;
    HIP_TRY(c, hipMemcpyAsync(d_theta, theta, nt * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = enqueue_fisher(c, W, d_theta, d_lnprob, d_fisher, c->stream))) return rc;
    HIP_TRY(c, hipMemcpyAsync(fisher, d_fisher, nf * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(lnprob, d_lnprob, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return VP_OK;
}

int vp_model_flux_jacobian(vp_ctx* c, int inst, int W, int D, const double* theta, double* out, int convolved) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    int rc = check_batch_args(c, W, D, theta, out);
    if (rc) return rc;
    if (inst < 0 || inst >= (int)c->inst.size()) return fail(c, VP_EINVAL, "vp_model_flux_jacobian: instrument index out of range");
    if ((rc = grad_refusals(c, "vp_model_flux_jacobian", "analytic Jacobian"))) return rc;
    if (W == 0) return VP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const int Wc = fisher_rows_per_pass(c, W, false);
    if ((rc = fisher_grow_jacobian(c, Wc))) return rc;
    auto& Fw = c->fisher;
    // theta of a pass | one zero per row: the prior is not consulted, every row counts as evaluable (a NaN in theta gives NaN rows)
    if ((rc = grad_grow(c, &Fw.io, &Fw.n_io, (size_t)Wc * D + Wc))) return rc;
    double* d_theta = Fw.io;
    double* d_zero = Fw.io + (size_t)Wc * D;
    Instrument& in = c->inst[inst];
    const size_t row = (size_t)D * in.dev.P;
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemsetAsync(d_zero, 0, (size_t)Wc * sizeof(double), s));
    for (int w0 = 0; w0 < W; w0 += Wc) {
        const int n = std::min(Wc, W - w0);
        HIP_TRY(c, hipMemcpyAsync(d_theta, theta + (size_t)w0 * D, (size_t)n * D * sizeof(double), hipMemcpyHostToDevice, s));
        const double* J = nullptr;
        if ((rc = enqueue_jacobian(c, in, n, d_theta, d_zero, convolved != 0, s, &J))) return rc;
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(out + (size_t)w0 * row, J, (size_t)n * row * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    return VP_OK;
}
