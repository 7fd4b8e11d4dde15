// capi_samplers.inc -- entry points: device-resident stretch-move and slice samplers (vp_stretch_run, vp_slice_run).
// A fragment of the ONE translation unit capi.hip (included there inside extern "C", in order; not a header of its own).
namespace {
// what both stretch entries ask of their arguments (`w`: the entry's name); the message is left in c
int stretch_check_args(vp_ctx* c, const std::string& w, int W, int nsteps, double a, const double* chain, const double* chain_lnprob,
                       int have_lnprob, const double* lnprob) {
    if (W < 2 || (W & 1)) return fail(c, VP_EINVAL, w + ": the number of walkers must be even and >= 2");
    if (nsteps < 0 || !(a > 1.0)) return fail(c, VP_EINVAL, w + ": nsteps must be >= 0 and a > 1");
    if ((chain == nullptr) != (chain_lnprob == nullptr)) return fail(c, VP_EINVAL, w + ": chain and chain_lnprob go together");
    for (int k = 0; have_lnprob && k < W; ++k)
        if (lnprob[k] != lnprob[k]) return fail(c, VP_ENAN, w + ": the initial lnprob holds NaN (Probability function returned NaN)");
    return VP_OK;
}
}  // namespace
static int multi_barrier(vp_multi* m);
static int multi_fail(vp_multi* m, int i, int rc);
// How a sampler that drives several contexts fails on slot i of them: that context gets the message; a vp_multi entry point
// (bad == NULL) returns through multi_fail ("device slot i: ..."), slice_run_impl tells its caller the slot, which does the same.
struct SlotFail {
    vp_multi* m; vp_ctx* const* cx; int* bad;
    int code(int i, int rc) const { if (!bad) return multi_fail(m, i, rc); *bad = i; return rc; }
    int operator()(int i, int rc, const std::string& msg) const { return code(i, fail(cx[i], rc, msg)); }
};
#define SLOT_TRY(F, i, expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return (F)((i), VP_EHIP, std::string(#expr) + ": " + hipGetErrorString(e__)); } while (0)

int vp_stretch_run(vp_ctx* c, int W, int D, double* pos, double* lnprob, int have_lnprob, int nsteps, double a,
                   uint64_t seed, uint64_t step0, double* chain, double* chain_lnprob, int64_t* naccepted) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    int rc = check_batch_args(c, W, D, pos, lnprob);
    if (rc || (rc = stretch_check_args(c, "vp_stretch_run", W, nsteps, a, chain, chain_lnprob, have_lnprob, lnprob))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = ensure_workspace(c, W))) return rc;
    hipStream_t s = c->stream;
    const int half = W / 2;
    const size_t row = (size_t)W * (D + 1);                       // doubles stored per step
    const size_t chunk = chain ? chain_chunk(nsteps, row) : 0;
    struct Dev { double *pos, *lp, *prop, *lpnew, *zz, *pos1, *lp1, *mail, *chain; long long* nacc; int *nan, *ver; size_t zeroed; } d;
    if ((rc = carve_scratch(c, [&](Arena& A) {
        d.pos = A.take<double>((size_t)W * D); d.lp = A.take<double>(W);
        d.prop = A.take<double>((size_t)half * D); d.lpnew = A.take<double>(half); d.zz = A.take<double>(half);
        d.pos1 = A.take<double>((size_t)W * D); d.lp1 = A.take<double>(W);     // the rows' second buffer (overlapped half-steps)
        // mailbox lines 2 x W x 8 (overlapped half-steps with D <= 6: row, lnprob, version in one 64-byte line)
        d.mail = A.take<double>(2 * (size_t)W * 8, 64);
        d.chain = A.take<double>(chunk * row);                     // chunk * (W*D) then chunk * W
        // nacc (W) | flags: [0] NaN, [1] a device-side wait gave up | versions (W): cleared by ONE memset
        d.nacc = A.take<long long>(W); d.nan = A.take<int>(16); d.ver = A.take<int>(W); d.zeroed = A.bytes_from(d.nacc);
    }))) return rc;
    HIP_TRY(c, hipMemcpyAsync(d.pos, pos, (size_t)W * D * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemsetAsync(d.nacc, 0, d.zeroed, s));
    if (have_lnprob) {
        HIP_TRY(c, hipMemcpyAsync(d.lp, lnprob, (size_t)W * sizeof(double), hipMemcpyHostToDevice, s));
    } else {
        // a walker that starts at NaN would never move (log u < NaN is false) and the run would still report success
        if ((rc = enqueue_lnprob(c, W, d.pos, d.lp, s))) return rc;
        hipLaunchKernelGGL(vp::nan_flag_kernel, dim3((W + 255) / 256), dim3(256), 0, s, d.lp, W, d.nan);
        int h_nan0 = 0;
        HIP_TRY(c, hipMemcpyAsync(&h_nan0, d.nan, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        if (h_nan0) return fail(c, VP_ENAN, "vp_stretch_run: the initial lnprob holds NaN (Probability function returned NaN)");
    }
    const int thr = 64;
    const int split = stretch_split(c, half);
    const bool one_launch = split >= 0;
    const bool fuse = W <= 1024 && !c->tune.no_fused_accept;   // accept + next proposal in one launch
    const int wthr = ((W + 63) / 64) * 64;
    bool have_prop = false;                                   // is the proposal of the coming pass already enqueued?
    // Overlapped half-steps: consecutive half-steps on two streams, each walker waiting for its partner's version word only
    // (StretchArgs::ovl).  Both launches must be able to sit on the CUs together -- a workgroup that waits holds its slot, and
    // the one it waits for must never be left without one: two half-ensembles of workgroups within what the CUs hold at once.
    bool ovl = false;
    if (one_launch && c->tune.stretch_overlap != 0 && nsteps > 0) {
        const int nt = split > 0 ? split_shape(c, split).waves : walker_tiles(c);
        const size_t wl = split > 0 ? split_shape(c, split).lds : walker_lds_bytes(c);
        const long per_cu = std::max(1, std::min((split > 0 ? 28 : 24) / std::max(1, nt), (int)(c->lds_limit / wl)));
        ovl = c->tune.stretch_overlap > 0 || (per_cu >= 2 && 2l * half * std::max(1, split) <= per_cu * (long)ctx_num_cus(c));
        if (ovl && !c->stream2) {
            if (hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess ||
                hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); ovl = false; }
        }
    }
    // mailbox lines (StretchArgs::ovl == 2): row, lnprob and version of a walker in one 64-byte line per buffer, packed here
    const bool mail = ovl && D <= 6 && c->tune.stretch_mailbox != 0;
    std::vector<double> h_mail;
    if (mail) {
        h_mail.assign(2 * (size_t)W * 8, 0.0);
        std::vector<double> lp0(W);
        if (have_lnprob) std::memcpy(lp0.data(), lnprob, (size_t)W * sizeof(double));
        else {
            HIP_TRY(c, hipMemcpyAsync(lp0.data(), d.lp, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipStreamSynchronize(s));
        }
        for (int w = 0; w < W; ++w) {
            std::memcpy(&h_mail[(size_t)w * 8], pos + (size_t)w * D, (size_t)D * sizeof(double));
            h_mail[(size_t)w * 8 + 6] = lp0[w];                    // ([7]: version 0 = all-zero bits)
        }
        HIP_TRY(c, hipMemcpyAsync(d.mail, h_mail.data(), h_mail.size() * sizeof(double), hipMemcpyHostToDevice, s));
    }
    hipStream_t s2 = ovl ? c->stream2 : s;
    // (whatever way this call ends -- an error return from the middle of the loop included -- nothing of it is left running on the
    //  second stream when the context's mutex is released)
    struct DrainSecond { hipStream_t q; bool on; ~DrainSecond() { if (on) (void)hipStreamSynchronize(q); } } drain_second{s2, ovl};
    if (ovl) {      // what the first stream has set up (rows, versions) before the second one's first launch
        HIP_TRY(c, hipEventRecord(c->ev_fork, s));
        HIP_TRY(c, hipStreamWaitEvent(s2, c->ev_fork, 0));
    }
    for (int done = 0; done < nsteps;) {
        const int n = chain ? (int)std::min<size_t>(chunk, (size_t)(nsteps - done)) : nsteps - done;
        for (int it = 0; it < n; ++it) {
            const uint64_t step = step0 + (uint64_t)(done + it);
            for (int h = 0; h < 2; ++h) {
                const int s0 = h ? half : 0, c0 = h ? 0 : half;
                if (one_launch) {
                    vp::StretchArgs sa{};
                    sa.pos = d.pos; sa.lp = d.lp; sa.nacc = d.nacc; sa.nanflag = d.nan;
                    sa.chain_pos = chain ? d.chain + (size_t)it * W * D : (double*)nullptr;
                    sa.chain_lp = chain ? d.chain + chunk * (size_t)W * D + (size_t)it * W : (double*)nullptr;
                    sa.a = a; sa.seed = seed; sa.step = step; sa.s0 = s0; sa.c0 = c0; sa.nC = half; sa.half = h;
                    if (ovl) {
                        // every walker has been updated k = done + it times when this step begins (the first half once more when
                        // h = 1): rows live in buffer (update count) & 1
                        const int k = done + it, t = 2 * k + h;
                        double* pb[2] = {mail ? d.mail : d.pos, mail ? d.mail + (size_t)W * 8 : d.pos1};
                        double* lb2[2] = {d.lp, d.lp1};
                        sa.ovl = mail ? 2 : 1; sa.need = t; sa.mine = t + 1; sa.ver = d.ver; sa.timeout = d.nan + 1;
                        sa.pos_x = pb[k & 1]; sa.lp_x = lb2[k & 1];
                        sa.pos_w = pb[(k + 1) & 1]; sa.lp_w = lb2[(k + 1) & 1];
                        sa.pos_c = pb[(h ? k + 1 : k) & 1];
                        launch_walker_stretch(c, half, sa, h ? s2 : s, h ? half : 0, split);
                    } else {
                        launch_walker_stretch(c, half, sa, s, 0, split);
                    }
                    continue;
                }
                if (!have_prop)
                    hipLaunchKernelGGL(vp::stretch_propose_kernel, dim3((half + thr - 1) / thr), dim3(thr), 0, s, d.pos, D, s0,
                                       half, c0, half, a, seed, step, h, d.prop, d.zz);
                if ((rc = enqueue_lnprob(c, half, d.prop, d.lpnew, s))) return rc;
                const bool store = chain && h == 1;
                double* cp = store ? d.chain + (size_t)it * W * D : (double*)nullptr;
                double* cl = store ? d.chain + chunk * (size_t)W * D + (size_t)it * W : (double*)nullptr;
                const bool last = (h == 1) && (done + it + 1 == nsteps);
                if (fuse && !last) {
                    vp::NextProposal nx;
                    nx.half = 1 - h; nx.s0 = nx.half ? half : 0; nx.c0 = nx.half ? 0 : half; nx.nS = half; nx.nC = half;
                    nx.step = h ? step + 1 : step;
                    hipLaunchKernelGGL(vp::stretch_accept_propose_kernel, dim3(1), dim3(wthr), 0, s, d.pos, d.lp, d.prop,
                                       d.lpnew, d.zz, W, D, s0, half, seed, step, h, d.nacc, d.nan, cp, cl, a, nx);
                    have_prop = true;
                } else {
                    hipLaunchKernelGGL(vp::stretch_accept_kernel, dim3((W + thr - 1) / thr), dim3(thr), 0, s, d.pos, d.lp, d.prop,
                                       d.lpnew, d.zz, W, D, s0, half, seed, step, h, d.nacc, d.nan, cp, cl);
                    have_prop = false;
                }
            }
        }
        HIP_TRY(c, hipGetLastError());
        if (ovl) {      // the second stream's half-steps of this chunk are done before the first stream copies anything out
            HIP_TRY(c, hipEventRecord(c->ev_join, s2));
            HIP_TRY(c, hipStreamWaitEvent(s, c->ev_join, 0));
        }
        if (chain) {
            HIP_TRY(c, hipMemcpyAsync(chain + (size_t)done * W * D, d.chain, (size_t)n * W * D * sizeof(double), hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipMemcpyAsync(chain_lnprob + (size_t)done * W, d.chain + chunk * (size_t)W * D, (size_t)n * W * sizeof(double),
                                      hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipStreamSynchronize(s));      // (the host waits: the next chunk's launches are enqueued behind the copies)
        }
        done += n;
    }
    std::vector<long long> h_nacc(W);
    int h_flags[2] = {0, 0};
    // (overlapped half-steps: after nsteps updates the rows are in buffer nsteps & 1)
    if (mail) {
        HIP_TRY(c, hipMemcpyAsync(h_mail.data(), d.mail + (size_t)(nsteps & 1) * W * 8, (size_t)W * 8 * sizeof(double), hipMemcpyDeviceToHost, s));
    } else {
        HIP_TRY(c, hipMemcpyAsync(pos, (ovl && (nsteps & 1)) ? d.pos1 : d.pos, (size_t)W * D * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(lnprob, (ovl && (nsteps & 1)) ? d.lp1 : d.lp, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipMemcpyAsync(h_nacc.data(), d.nacc, (size_t)W * sizeof(long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(h_flags, d.nan, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (mail)
        for (int w = 0; w < W; ++w) {
            std::memcpy(pos + (size_t)w * D, &h_mail[(size_t)w * 8], (size_t)D * sizeof(double));
            lnprob[w] = h_mail[(size_t)w * 8 + 6];
        }
    if (h_flags[1]) return fail(c, VP_EHIP, "vp_stretch_run: a workgroup's wait for its partner's half-step gave up (overlapped half-steps)");
    if (naccepted) for (int w = 0; w < W; ++w) naccepted[w] += (int64_t)h_nacc[w];
    if (h_flags[0]) return fail(c, VP_ENAN, "vp_stretch_run: Probability function returned NaN");
    return VP_OK;
}

// vp_slice_run on G >= 1 contexts (called with every context's mutex held).  G = 1 is the single-GPU sampler.  With G > 1
// (vp_multi_slice_run) every context holds the whole sampler state and runs the SAME control kernels on it -- begin,
// init, update, tune are deterministic functions of that state -- while each round's lnprob batch of B trial rows is cut
// into blocks of ceil(B / G) rows, one per context, evaluated with the launch structure the whole batch would get
// (LaunchPlan::Wp), and written into EVERY replica's result vector (one double per row through peer-mapped pointers), followed
// by the event barrier.  The replicas therefore stay identical bit for bit, and equal to the single-context run.
namespace { __global__ void scatter_rows_kernel(const double* __restrict__ src, int n, int lo, vp::Replicas R) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const double v = src[k];
    for (int r = 0; r < R.n; ++r) R.lp[r][lo + k] = v;        // (R.lp: the replicas' row-result vectors)
} }

static int slice_run_impl(vp_multi* m, vp_ctx* const* cx, int G, int W, int D, double* pos, double* lnprob, int have_lnprob,
                          int nsteps, double* mu, int* tune, double tolerance, int patience, int maxsteps, uint64_t seed,
                          uint64_t step0, double* chain, double* chain_lnprob, double* mu_history, int64_t* n_evals, int* bad) {
    *bad = 0;
    vp_ctx* c = cx[0];
    int rc;
    const SlotFail F{m, cx, bad};
    if (W < 4 || (W & 1) || W > 2 * vp::SLICE_MAX_HALF)
        return F(0, VP_EINVAL, "vp_slice_run: the number of walkers must be even, >= 4 and <= " + std::to_string(2 * vp::SLICE_MAX_HALF));
    if (nsteps < 0 || !mu || !(*mu > 0.0) || !tune || maxsteps < 1 || patience < 1 || !(tolerance >= 0.0))
        return F(0, VP_EINVAL, "vp_slice_run: nsteps >= 0, mu > 0, maxsteps >= 1, patience >= 1, tolerance >= 0 and non-NULL mu/tune required");
    if ((chain == nullptr) != (chain_lnprob == nullptr)) return F(0, VP_EINVAL, "vp_slice_run: chain and chain_lnprob go together");
    const int half = W / 2;
    // rows of every round's lnprob batch (the round kernel keeps one slice parameter per row in LDS: <= 4096 rows)
    const int B = std::min(2 * vp::SLICE_MAX_HALF, std::max(2, std::min(8, c->tune.slice_rows)) * half);
    const int per = (B + G - 1) / G;
    // A segment = the iterations the device works through on its own (slice_round_kernel) before the host collects the
    // chain: bounded by the chain chunk (256 MB) and by the table of random splits (64 MB).
    const size_t row = (size_t)W * (D + 1);
    size_t seg = std::min<size_t>((size_t)std::max(nsteps, 1), ((size_t)64 << 20) / ((size_t)W * sizeof(int)));
    if (chain) seg = std::min(seg, std::max<size_t>(1, ((size_t)256 << 20) / (row * sizeof(double))));
    if (c->tune.slice_seg > 0) seg = std::min(seg, (size_t)c->tune.slice_seg);
    struct Dev { double *pos, *lp, *trial, *rows, *mu, *muhist, *blk, *chain; long long* ll; int *perm, *nact, *prog; size_t zeroed; vp::SliceState st; vp::SliceCounters cn; hipStream_t s; };
    std::vector<Dev> dv(G);
    const double h_mu[4] = {*mu, *tune > 0 ? (double)(*tune - 1) : 0.0, *tune ? 1.0 : 0.0, 0.0};   // `tune` carries the state across calls
    for (int i = 0; i < G; ++i) {
        vp_ctx* ci = cx[i];
        SLOT_TRY(F, i, hipSetDevice(ci->device));
        if ((rc = ensure_workspace(ci, std::max(W, B)))) return F.code(i, rc);
        Dev& d = dv[i];
        d.s = ci->stream;
        if ((rc = carve_scratch(ci, [&](Arena& A) {         // every replica's state: the doubles first, then the integer state
            d.pos = A.take<double>((size_t)W * D); d.lp = A.take<double>(W);
            d.trial = A.take<double>(2 * (size_t)B * D); d.rows = A.take<double>(2 * (size_t)B);    // (each twice: the rounds alternate)
            d.st.X0 = A.take<double>((size_t)half * D); d.st.eta = A.take<double>((size_t)half * D);
            d.st.Z0 = A.take<double>(half); d.st.L = A.take<double>(half); d.st.R = A.take<double>(half);
            d.st.T = A.take<double>((size_t)half * vp::SLICE_MAXC);
            d.mu = A.take<double>(4); d.muhist = A.take<double>(std::max(nsteps, 1));       // (mu: 3 used)
            d.blk = A.take<double>(per);                                // this context's block of a round's results
            d.chain = A.take<double>(i == 0 && chain ? seg * row : 0);  // the chain segment: replica 0
            d.ll = A.take<long long>(4);                                // n_evals, nexp, ncon, (pad)
            d.st.J = A.take<int>(half); d.st.K = A.take<int>(half); d.st.phase = A.take<int>(half); d.st.sides = A.take<int>(half);
            d.st.nshr = A.take<int>(half); d.st.row = A.take<int>(half); d.st.widx = A.take<int>(half);
            // n_active, nanflag, ncand, (pad) | prog (slice_kernels.h SliceRun::prog): cleared by ONE memset
            d.nact = A.take<int>(8); d.prog = A.take<int>(8); d.zeroed = A.bytes_from(d.nact);
            d.perm = A.take<int>(seg * (size_t)W);                      // (seg, W)
        }))) return F.code(i, rc);
        d.cn = vp::SliceCounters{d.nact, d.ll, d.ll + 1, d.ll + 2, d.nact + 1, d.nact + 2, d.mu};
        SLOT_TRY(F, i, hipMemcpyAsync(d.pos, pos, (size_t)W * D * sizeof(double), hipMemcpyHostToDevice, d.s));
        SLOT_TRY(F, i, hipMemcpyAsync(d.mu, h_mu, sizeof(h_mu), hipMemcpyHostToDevice, d.s));
        SLOT_TRY(F, i, hipMemsetAsync(d.ll, 0, 4 * sizeof(long long), d.s));
        SLOT_TRY(F, i, hipMemsetAsync(d.nact, 0, d.zeroed, d.s));
        if (have_lnprob) SLOT_TRY(F, i, hipMemcpyAsync(d.lp, lnprob, (size_t)W * sizeof(double), hipMemcpyHostToDevice, d.s));
        else if ((rc = enqueue_lnprob(ci, W, d.pos, d.lp, d.s))) return F.code(i, rc);     // (every replica: once per run)
    }
    {   // the start state must be finite everywhere (zeus: "Invalid walker initial positions")
        std::vector<double> h_lp(W);
        SLOT_TRY(F, 0, hipSetDevice(c->device));
        SLOT_TRY(F, 0, hipMemcpyAsync(h_lp.data(), dv[0].lp, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, dv[0].s));
        SLOT_TRY(F, 0, hipStreamSynchronize(dv[0].s));
        for (int w = 0; w < W; ++w)
            if (!(std::fabs(h_lp[w]) <= 1.79e308))
                return F(0, VP_ENAN, "vp_slice_run: the initial lnprob of walker " + std::to_string(w) + " is not finite");
    }
    // two words of mapped host memory that replica 0's round kernel keeps up to date: rounds consumed, done / error
    volatile int* h_words = nullptr;
    int* d_words = nullptr;
    {
        SLOT_TRY(F, 0, hipSetDevice(c->device));
        if (!c->h_done) {
            if (hipHostMalloc((void**)&c->h_done, 64, hipHostMallocMapped) != hipSuccess) { c->h_done = nullptr; (void)hipGetLastError(); }
            else std::memset(c->h_done, 0, 64);
        }
        void* dptr = nullptr;
        if (c->h_done && hipHostGetDevicePointer(&dptr, c->h_done, 0) == hipSuccess) {
            h_words = reinterpret_cast<volatile int*>(c->h_done + 8);
            d_words = reinterpret_cast<int*>(static_cast<uint32_t*>(dptr) + 8);
        } else {
            (void)hipGetLastError();
        }
    }
    int parity = 0;                                  // which of the two row-result vectors the coming round fills (G > 1)
    int tb = 0;                                      // which of the two trial batches the coming round evaluates
    if (G > 1 && (rc = multi_barrier(m))) return rc;
    vp::SliceRun P{};
    P.W = W; P.half = half; P.D = D; P.batch_rows = B; P.maxsteps = maxsteps; P.patience = patience;
    P.round_limit = (int)std::min<long long>(4ll * maxsteps + 4096, 1ll << 30);
    P.gamma0 = 2.38 / std::sqrt(2.0 * (double)D);
    P.tolerance = tolerance; P.seed = seed;
    auto launch_round = [&](int i, int start) {
        const Dev& d = dv[i];
        vp::SliceRun Pi = P;
        // (start: the first batch goes into buffer tb; a round consumes buffer tb ^ 1 -- flipped by then -- and fills tb)
        Pi.pos = d.pos; Pi.lp = d.lp; Pi.perm_tab = d.perm; Pi.prog = d.prog;
        Pi.trial = d.trial + (size_t)tb * B * D;
        Pi.trial_in = d.trial + (size_t)(tb ^ 1) * B * D;
        Pi.host = i == 0 ? d_words : nullptr;
        Pi.chain = i == 0 && chain ? d.chain : nullptr;
        Pi.chain_lp = i == 0 && chain ? d.chain + seg * (size_t)W * D : nullptr;
        Pi.mu_hist = d.muhist + (P.step_base - step0);
        hipLaunchKernelGGL(vp::slice_round_kernel, dim3(1), dim3(1024), 0, d.s, Pi, d.st, d.cn, d.rows + (G > 1 ? (size_t)(parity ^ 1) * B : 0), start);
    };
    // one round: the lnprob of the B trial rows (sharded when G > 1), then the round kernel on every replica
    auto round = [&]() -> int {
        const size_t roff = G > 1 ? (size_t)parity * B : 0;
        vp::Replicas R{};
        R.n = G;
        for (int i = 0; i < G; ++i) { R.pos[i] = nullptr; R.lp[i] = dv[i].rows + roff; }
        for (int i = 0; i < G; ++i) {
            vp_ctx* ci = cx[i];
            const Dev& d = dv[i];
            SLOT_TRY(F, i, hipSetDevice(ci->device));
            if (G == 1) {
                if ((rc = enqueue_lnprob(ci, B, d.trial + (size_t)tb * B * D, d.rows, d.s))) return F.code(i, rc);
            } else {
                const auto [lo, n] = block_of(i, per, B);
                if (n <= 0) continue;
                if ((rc = enqueue_lnprob(ci, n, d.trial + ((size_t)tb * B + lo) * D, d.blk, d.s, B))) return F.code(i, rc);
                hipLaunchKernelGGL(scatter_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, d.s, d.blk, n, lo, R);
            }
        }
        // every block's results are in every replica before any replica consumes them.  (The other hazard -- a block of
        // the NEXT round landing in a vector a replica's round kernel is still reading -- cannot occur: the rounds alternate
        // between two vectors, and a replica's kernel of round r precedes, on its own stream, the event it records in
        // round r + 1, which every scatter of round r + 2 waits for.)
        if (G > 1 && (rc = multi_barrier(m))) return rc;
        parity ^= 1;
        tb ^= 1;
        for (int i = 0; i < G; ++i) {
            SLOT_TRY(F, i, hipSetDevice(cx[i]->device));
            launch_round(i, 0);
        }
        return VP_OK;
    };
    const int ahead = 8;                             // rounds the host keeps enqueued beyond the last one it has seen consumed
    for (int done = 0; done < nsteps;) {
        const int n = (int)std::min<size_t>(seg, (size_t)(nsteps - done));
        P.n = n;
        P.step_base = step0 + (uint64_t)done;
        if (h_words) { h_words[0] = 0; h_words[1] = 0; }
        for (int i = 0; i < G; ++i) {
            SLOT_TRY(F, i, hipSetDevice(cx[i]->device));
            hipLaunchKernelGGL(vp::slice_perm_kernel, dim3(n), dim3(1024), 0, dv[i].s, W, seed, P.step_base, dv[i].perm);
            launch_round(i, 1);
        }
        int enq = 0, h_prog[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        auto t_seen = std::chrono::steady_clock::now();
        int last_seen = -1, idle = 0;
        for (;;) {
            if (h_words) {
                if (__atomic_load_n(const_cast<int*>(h_words + 1), __ATOMIC_ACQUIRE)) break;
                const int seen = __atomic_load_n(const_cast<int*>(h_words), __ATOMIC_RELAXED);
                if (enq - seen >= ahead) {           // far enough ahead: wait for the device (and notice a stream that died)
                    __builtin_ia32_pause();
                    if (seen != last_seen) { last_seen = seen; t_seen = std::chrono::steady_clock::now(); idle = 0; }
                    else if (++idle > 20000) { std::this_thread::sleep_for(std::chrono::microseconds(20)); }   // (rounds of milliseconds: big models)
                    else if (std::chrono::steady_clock::now() - t_seen > std::chrono::seconds(5)) {
                        SLOT_TRY(F, 0, hipSetDevice(c->device));
                        const hipError_t q = hipStreamQuery(dv[0].s);
                        if (q != hipErrorNotReady) {     // the queue ran dry (or failed) without the word moving
                            if (q != hipSuccess) { (void)hipGetLastError(); return F(0, VP_EHIP, std::string("vp_slice_run: ") + hipGetErrorString(q)); }
                            if (!__atomic_load_n(const_cast<int*>(h_words + 1), __ATOMIC_ACQUIRE) &&
                                __atomic_load_n(const_cast<int*>(h_words), __ATOMIC_RELAXED) == seen) h_words = nullptr;   // word not delivered: poll by copy
                        }
                        t_seen = std::chrono::steady_clock::now();
                    }
                    continue;
                }
                if ((rc = round())) return rc;
                ++enq;
            } else {                                 // no mapped word: look at the device's state every few rounds
                for (int r = 0; r < ahead; ++r)
                    if ((rc = round())) return rc;
                SLOT_TRY(F, 0, hipSetDevice(c->device));
                SLOT_TRY(F, 0, hipMemcpyAsync(h_prog, dv[0].prog, sizeof(h_prog), hipMemcpyDeviceToHost, dv[0].s));
                SLOT_TRY(F, 0, hipStreamSynchronize(dv[0].s));
                if (h_prog[2]) break;
            }
        }
        // the segment is over on the device: drain what is still enqueued (launches that return at once), look at the outcome
        for (int i = G - 1; i >= 0; --i) {
            SLOT_TRY(F, i, hipSetDevice(cx[i]->device));
            if (i == 0) SLOT_TRY(F, 0, hipMemcpyAsync(h_prog, dv[0].prog, sizeof(h_prog), hipMemcpyDeviceToHost, dv[0].s));
            SLOT_TRY(F, i, hipStreamSynchronize(dv[i].s));
        }
        SLOT_TRY(F, 0, hipGetLastError());
        if (h_prog[3] == 1) return F(0, VP_ENAN, "vp_slice_run: Log Probability returned NaN");
        if (h_prog[3]) return F(0, VP_ESTATE, "vp_slice_run: a slice did not terminate");
        if (chain) {
            SLOT_TRY(F, 0, hipMemcpyAsync(chain + (size_t)done * W * D, dv[0].chain, (size_t)n * W * D * sizeof(double), hipMemcpyDeviceToHost, dv[0].s));
            SLOT_TRY(F, 0, hipMemcpyAsync(chain_lnprob + (size_t)done * W, dv[0].chain + seg * (size_t)W * D, (size_t)n * W * sizeof(double),
                                         hipMemcpyDeviceToHost, dv[0].s));
            SLOT_TRY(F, 0, hipStreamSynchronize(dv[0].s));
        }
        if (G > 1 && (rc = multi_barrier(m))) return rc;
        done += n;
    }
    SLOT_TRY(F, 0, hipSetDevice(c->device));
    double h_mu_out[4];
    long long h_ll[4];
    SLOT_TRY(F, 0, hipMemcpyAsync(pos, dv[0].pos, (size_t)W * D * sizeof(double), hipMemcpyDeviceToHost, dv[0].s));
    SLOT_TRY(F, 0, hipMemcpyAsync(lnprob, dv[0].lp, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, dv[0].s));
    SLOT_TRY(F, 0, hipMemcpyAsync(h_mu_out, dv[0].mu, sizeof(h_mu_out), hipMemcpyDeviceToHost, dv[0].s));
    SLOT_TRY(F, 0, hipMemcpyAsync(h_ll, dv[0].ll, sizeof(h_ll), hipMemcpyDeviceToHost, dv[0].s));
    if (mu_history && nsteps > 0) SLOT_TRY(F, 0, hipMemcpyAsync(mu_history, dv[0].muhist, (size_t)nsteps * sizeof(double), hipMemcpyDeviceToHost, dv[0].s));
    SLOT_TRY(F, 0, hipStreamSynchronize(dv[0].s));
    for (int i = 1; i < G; ++i) {                                    // the other replicas have nothing left in flight either
        SLOT_TRY(F, i, hipSetDevice(cx[i]->device));
        SLOT_TRY(F, i, hipStreamSynchronize(dv[i].s));
    }
    *mu = h_mu_out[0];
    *tune = h_mu_out[2] != 0.0 ? 1 + (int)h_mu_out[1] : 0;
    if (n_evals) *n_evals += (int64_t)h_ll[0];
    return VP_OK;
}

int vp_slice_run(vp_ctx* c, int W, int D, double* pos, double* lnprob, int have_lnprob, int nsteps, double* mu,
                 int* tune, double tolerance, int patience, int maxsteps, uint64_t seed, uint64_t step0,
                 double* chain, double* chain_lnprob, double* mu_history, int64_t* n_evals) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    int rc = check_batch_args(c, W, D, pos, lnprob);
    if (rc) return rc;
    int bad = 0;
    vp_ctx* cx[1] = {c};
    return slice_run_impl(nullptr, cx, 1, W, D, pos, lnprob, have_lnprob, nsteps, mu, tune, tolerance, patience, maxsteps, seed, step0,
                          chain, chain_lnprob, mu_history, n_evals, &bad);
}

#ifdef VP_STAMPS
// diagnostic build only: the far-field workspace of the last lnprob launch (doubles)
extern "C" int vp_debug_read_ff(vp_ctx* c, double* out, long n) {
    if (!c || !c->d_ff) return -1;
    hipDeviceSynchronize();
    return hipMemcpy(out, c->d_ff, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
// diagnostic build only: thread 0's clock at the phases of the slice sampler's round kernels (round, stage)
extern "C" int vp_debug_read_slice_stamps(long long* out, int n) {
    const size_t bytes = sizeof(long long) * (size_t)std::min(n, vp::SLICE_STAMP_ROUNDS * vp::SLICE_STAMP_STAGES);
    hipDeviceSynchronize();
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(vp::g_slice_stamps), bytes, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
extern "C" int vp_debug_host_stamps(double* out8) { std::memcpy(out8, g_host_stamps, sizeof g_host_stamps); return 0; }
// diagnostic build only: the walker kernel's phase stamps of the last launch (shader clock), (walker, wave, stage)
extern "C" int vp_debug_read_stamps(long long* out, int n) {
    const size_t bytes = sizeof(long long) * (size_t)std::min(n, vp::STAMP_W * vp::STAMP_WAVES * vp::STAMP_STAGES);
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(vp::g_stamps), bytes, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif

