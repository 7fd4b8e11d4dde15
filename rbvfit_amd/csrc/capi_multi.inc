// capi_multi.inc -- entry points: several device contexts driven by one process (vp_multi_*).
// A fragment of the ONE translation unit capi.hip (included there inside extern "C", in order; not a header of its own).
// ---- several GPUs from ONE process, no torch / RCCL needed (SURVEY 8b: vp_ctx_create(n_devices, device_ids)) ------
// Walkers are independent, so a batch is cut into contiguous blocks of ceil(W / G) theta rows, one per context;
// every context holds the same static data; all blocks are enqueued before any is waited for, and each block's
// lnprob lands directly in its slice of the caller's output -- the "gather" of this path is G device-to-host
// copies into one host vector (the RCCL all-gather is for device-resident ensembles, rbvfit_amd/dist.py).
int vp_multi_create(vp_multi** out, int n_devices, const int* device_ids) {
    if (!out) return fail(nullptr, VP_EINVAL, "out is NULL");
    *out = nullptr;
    if (n_devices <= 0 || !device_ids) return fail(nullptr, VP_EINVAL, "vp_multi_create: n_devices must be positive and device_ids non-NULL");
    vp_multi* m = new (std::nothrow) vp_multi();
    if (!m) return fail(nullptr, VP_ENOMEM, "out of host memory");
    for (int i = 0; i < n_devices; ++i) {
        vp_ctx* c = nullptr;
        const int rc = vp_ctx_create(&c, device_ids[i]);
        if (rc) {                                   // (g_create_error holds the reason)
            for (vp_ctx* p : m->ctx) vp_ctx_destroy(p);
            delete m;
            return rc;
        }
        m->ctx.push_back(c);
    }
    // the contexts write into each other's ensembles (vp_multi_stretch_run): peer access between distinct devices
    for (vp_ctx* a : m->ctx)
        for (vp_ctx* b : m->ctx)
            if (a->device != b->device && hipSetDevice(a->device) == hipSuccess) {
                const hipError_t pe = hipDeviceEnablePeerAccess(b->device, 0);
                if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) m->no_peer = true;
                (void)hipGetLastError();
            }
    *out = m;
    return VP_OK;
}

int vp_multi_destroy(vp_multi* m) {
    if (!m) return VP_OK;
    for (size_t i = 0; i < m->ev.size(); ++i) {
        hipSetDevice(m->ctx[i]->device);
        hipEventDestroy(m->ev[i]);
    }
    for (vp_ctx* c : m->ctx) vp_ctx_destroy(c);
    delete m;
    return VP_OK;
}

int vp_multi_n_devices(const vp_multi* m) { return m ? (int)m->ctx.size() : 0; }
vp_ctx* vp_multi_ctx(vp_multi* m, int i) { return (m && i >= 0 && i < (int)m->ctx.size()) ? m->ctx[i] : nullptr; }
const char* vp_multi_last_error(const vp_multi* m) { return m ? m->err.c_str() : g_create_error.c_str(); }

static int multi_fail(vp_multi* m, int i, int rc) {
    m->err = "device slot " + std::to_string(i) + ": " + vp_last_error(m->ctx[i]);
    return rc;
}

static int multi_broken(vp_multi* m) {
    m->err = "this vp_multi is unusable: an earlier vp_multi_set_bounds / vp_multi_add_instrument failed on one device and could not be undone on the others";
    return VP_ESTATE;
}

// (internal) drop the instrument added last to one context: the undo step of vp_multi_add_instrument
static int ctx_pop_instrument(vp_ctx* c) {
    CtxGuard g(c);
    if (c->inst.empty()) return VP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize());
    for (void* p : c->inst.back().allocs) hipFree(p);
    c->inst.pop_back();
    c->meta_dirty = true;
    return VP_OK;
}

int vp_multi_set_bounds(vp_multi* m, int D, const double* lb, const double* ub) {
    if (!m) return VP_EINVAL;
    std::lock_guard<std::mutex> g(m->mu);
    if (m->broken) return multi_broken(m);
    // what the contexts hold now (they are kept identical), to put back should a later context fail
    std::vector<double> old_lb, old_ub;
    int oldD = 0;
    {
        vp_ctx* c0 = m->ctx[0];
        std::lock_guard<std::mutex> g0(c0->mu);
        oldD = c0->D; old_lb = c0->h_lb; old_ub = c0->h_ub;
    }
    for (size_t i = 0; i < m->ctx.size(); ++i) {
        const int rc = vp_set_bounds(m->ctx[i], D, lb, ub);
        if (!rc) continue;
        multi_fail(m, (int)i, rc);
        for (size_t k = 0; k < i; ++k) {                 // undo on the contexts already changed
            if (oldD <= 0 || vp_set_bounds(m->ctx[k], oldD, old_lb.data(), old_ub.data()) != VP_OK) m->broken = true;
        }
        return rc;
    }
    return VP_OK;
}

int vp_multi_add_instrument(vp_multi* m, int P, const double* wave, const double* flux, const double* inv_sigma2,
                            const double* log_inv_sigma2, int L, const double* lambda0, const double* gamma,
                            const double* f, const double* zfac, const int32_t* N_idx, const int32_t* b_idx,
                            const int32_t* v_idx, int K, const double* taps, int lsf_mode, int voigt_method,
                            int* inst_index) {
    if (!m) return VP_EINVAL;
    std::lock_guard<std::mutex> g(m->mu);
    if (m->broken) return multi_broken(m);
    for (size_t i = 0; i < m->ctx.size(); ++i) {
        const int rc = vp_add_instrument(m->ctx[i], P, wave, flux, inv_sigma2, log_inv_sigma2, L, lambda0, gamma, f, zfac, N_idx, b_idx,
                                         v_idx, K, taps, lsf_mode, voigt_method, inst_index);
        if (!rc) continue;
        multi_fail(m, (int)i, rc);                       // (argument errors fail on the first context: nothing to undo)
        for (size_t k = 0; k < i; ++k)
            if (ctx_pop_instrument(m->ctx[k]) != VP_OK) m->broken = true;
        return rc;
    }
    return VP_OK;
}

int vp_multi_lnprob_batch(vp_multi* m, int W, int D, const double* theta, double* out) {
    if (!m) return VP_EINVAL;
    std::lock_guard<std::mutex> g(m->mu);
    if (m->broken) return multi_broken(m);
    if (W < 0 || (W > 0 && (!theta || !out))) { m->err = "vp_multi_lnprob_batch: bad batch"; return VP_EINVAL; }
    const int G = (int)m->ctx.size();
    const int per = W > 0 ? (W + G - 1) / G : 0;
    std::vector<std::unique_lock<std::mutex>> locks;
    std::vector<char> begun(G, 0);                     // whose batch is in flight (its pinned buffer exists and will be written)
    int rc = VP_OK;
    for (int i = 0; i < G && !rc; ++i) {               // every block in flight before any wait
        const auto [lo, n] = block_of(i, per, W);
        vp_ctx* c = m->ctx[i];
        locks.emplace_back(c->mu);
        prearm_cancel(c);
        if ((rc = check_batch_args(c, n, D, theta, out))) { multi_fail(m, i, rc); break; }
        if (n <= 0) continue;
        if ((rc = lnprob_host_begin(c, n, D, theta + (size_t)lo * D))) multi_fail(m, i, rc);
        else begun[i] = 1;
    }
    // drain what was started (also when a later block failed); `out` is written only when every block succeeded
    for (int i = 0; i < G; ++i) {
        if (!begun[i]) continue;
        vp_ctx* c = m->ctx[i];
        if (host_wait(c) != VP_OK && !rc) rc = multi_fail(m, i, VP_EHIP);
    }
    if (rc) return rc;
    for (int i = 0; i < G; ++i) {
        if (!begun[i]) continue;
        const auto [lo, n] = block_of(i, per, W);
        std::memcpy(out + lo, m->ctx[i]->h_pinned + (size_t)n * D, (size_t)n * sizeof(double));
    }
    return VP_OK;
}

// All G streams wait for all G streams: G event records + G (G - 1) stream waits, no host synchronisation.
static int multi_barrier(vp_multi* m) {
    const int G = (int)m->ctx.size();
    for (int g = 0; g < G; ++g) {
        vp_ctx* c = m->ctx[g];
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipEventRecord(m->ev[g], c->stream));
    }
    for (int g = 0; g < G; ++g) {
        vp_ctx* c = m->ctx[g];
        HIP_TRY(c, hipSetDevice(c->device));
        for (int h = 0; h < G; ++h)
            if (h != g) HIP_TRY(c, hipStreamWaitEvent(c->stream, m->ev[h], 0));
    }
    return VP_OK;
}

// (called with m->mu held) What the sharded samplers check and set up before anything else: a usable vp_multi whose devices map each
// other's memory, every context locked (`locks`) with its waiting launch sent away, a batch every context accepts, the barrier's events.
static int multi_sampler_enter(vp_multi* m, const char* who, int W, int D, const double* pos, const double* lnprob,
                               std::vector<std::unique_lock<std::mutex>>& locks) {
    if (m->broken) return multi_broken(m);
    const int G = (int)m->ctx.size();
    if (G > vp::MAX_REPLICAS) { m->err = std::string(who) + ": at most " + std::to_string(vp::MAX_REPLICAS) + " device contexts"; return VP_EINVAL; }
    if (m->no_peer) { m->err = std::string(who) + ": the devices cannot map each other's memory (no peer access)"; return VP_ESTATE; }
    for (int i = 0; i < G; ++i) { locks.emplace_back(m->ctx[i]->mu); prearm_cancel(m->ctx[i]); }
    for (int i = 0; i < G; ++i)
        if (int rc = check_batch_args(m->ctx[i], W, D, pos, lnprob)) return multi_fail(m, i, rc);
    for (int i = (int)m->ev.size(); i < G; ++i) {
        hipEvent_t e;
        if (hipSetDevice(m->ctx[i]->device) != hipSuccess || hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
            return multi_fail(m, i, fail(m->ctx[i], VP_EHIP, "hipEventCreate failed"));
        m->ev.push_back(e);
    }
    return VP_OK;
}

// One ensemble, G device contexts (BASELINE config 4: "2048 zeus walkers sharded over 8 GPUs"; vfit_mcmc.py:425-440,
// 536-540 fans ONE ensemble over its workers): see csrc/sampler_kernels.h.  Per half-step every context runs its block of
// the active half -- one walker_kernel launch where vp_stretch_run would use one for the whole half, else propose ->
// lnprob launches -> accept -- with the launch structure chosen as for the whole half (LaunchPlan::Wp), so every row gets
// the bits a single context gives it; then the event barrier.  Chain: replica 0 keeps it.
int vp_multi_stretch_run(vp_multi* m, int W, int D, double* pos, double* lnprob, int have_lnprob, int nsteps, double a,
                         uint64_t seed, uint64_t step0, double* chain, double* chain_lnprob, int64_t* naccepted) {
    if (!m) return VP_EINVAL;
    std::lock_guard<std::mutex> g(m->mu);
    std::vector<std::unique_lock<std::mutex>> locks;
    int rc = multi_sampler_enter(m, "vp_multi_stretch_run", W, D, pos, lnprob, locks);
    if (rc) return rc;
    const int G = (int)m->ctx.size();
    vp_ctx* c0 = m->ctx[0];
    const SlotFail F{m, m->ctx.data(), nullptr};
    if ((rc = stretch_check_args(c0, "vp_multi_stretch_run", W, nsteps, a, chain, chain_lnprob, have_lnprob, lnprob))) return F.code(0, rc);
    const int half = W / 2, per = (half + G - 1) / G;
    bool one_device = true;
    for (int i = 1; i < G; ++i) one_device = one_device && m->ctx[i]->device == c0->device;
    const bool flags_mode = c0->tune.multi_sync > 0;
    const size_t row = (size_t)W * (D + 1);
    const size_t chunk = chain ? chain_chunk(nsteps, row) : 0;
    struct Dev { double *pos, *lp, *prop, *lpnew, *zz, *chain; long long* nacc; int *nan, *flags, *timeout; unsigned int* done; size_t zeroed; };
    std::vector<Dev> dv(G);
    for (int i = 0; i < G; ++i) {
        vp_ctx* c = m->ctx[i];
        SLOT_TRY(F, i, hipSetDevice(c->device));
        if ((rc = ensure_workspace(c, std::max(W, per)))) return F.code(i, rc);
        Dev& d = dv[i];
        if ((rc = carve_scratch(c, [&](Arena& A) {
            d.pos = A.take<double>((size_t)W * D); d.lp = A.take<double>(W);
            d.prop = A.take<double>((size_t)per * D); d.lpnew = A.take<double>(per); d.zz = A.take<double>(per);
            // chain chunk (flags mode: every context keeps the rows of ITS walkers; events mode: replica 0 snapshots the ensemble)
            d.chain = A.take<double>((flags_mode || i == 0) ? chunk * row : 0);
            // nacc (W) | nanflag | flags | done (PUB_GROUPS + 1 counters) | timeout: cleared by ONE memset
            d.nacc = A.take<long long>(W); d.nan = A.take<int>(1); d.flags = A.take<int>(vp::MAX_REPLICAS);
            d.done = A.take<unsigned int>(vp::PUB_GROUPS + 1); d.timeout = A.take<int>(1); d.zeroed = A.bytes_from(d.nacc);
        }))) return F.code(i, rc);
        SLOT_TRY(F, i, hipMemcpyAsync(d.pos, pos, (size_t)W * D * sizeof(double), hipMemcpyHostToDevice, c->stream));
        SLOT_TRY(F, i, hipMemsetAsync(d.nacc, 0, d.zeroed, c->stream));
        if (have_lnprob) SLOT_TRY(F, i, hipMemcpyAsync(d.lp, lnprob, (size_t)W * sizeof(double), hipMemcpyHostToDevice, c->stream));
        else {
            // every replica evaluates the whole start state itself (once per run; the same launches as vp_stretch_run's)
            if ((rc = enqueue_lnprob(c, W, d.pos, d.lp, c->stream))) return F.code(i, rc);
            hipLaunchKernelGGL(vp::nan_flag_kernel, dim3((W + 255) / 256), dim3(256), 0, c->stream, d.lp, W, d.nan);
        }
    }
    if (!have_lnprob) {
        int h_nan0 = 0;
        SLOT_TRY(F, 0, hipSetDevice(c0->device));
        SLOT_TRY(F, 0, hipMemcpyAsync(&h_nan0, dv[0].nan, sizeof(int), hipMemcpyDeviceToHost, c0->stream));
        SLOT_TRY(F, 0, hipStreamSynchronize(c0->stream));
        if (h_nan0) return F(0, VP_ENAN, "vp_multi_stretch_run: the initial lnprob holds NaN (Probability function returned NaN)");
    }
    // every replica's start state (and its zeroed flags) is in place before any kernel of the run starts
    for (int i = 0; i < G; ++i) {
        vp_ctx* c = m->ctx[i];
        SLOT_TRY(F, i, hipSetDevice(c->device));
        SLOT_TRY(F, i, hipStreamSynchronize(c->stream));
    }
    const int thr = 64;
    std::vector<double> h_chunk;                       // flags mode: one context's chain chunk on its way to the caller's arrays
    int seq = 0;                                       // half-steps of this call so far
    for (int done = 0; done < nsteps;) {
        const int n = chain ? (int)std::min<size_t>(chunk, (size_t)(nsteps - done)) : nsteps - done;
        for (int it = 0; it < n; ++it) {
            const uint64_t step = step0 + (uint64_t)(done + it);
            for (int h = 0; h < 2; ++h) {
                const int s0 = h ? half : 0, cc0 = h ? 0 : half;
                ++seq;
                for (int i = 0; i < G; ++i) {
                    vp_ctx* c = m->ctx[i];
                    const auto [k0, nk] = block_of(i, per, half);
                    SLOT_TRY(F, i, hipSetDevice(c->device));
                    const Dev& d = dv[i];
                    vp::Replicas R{};
                    R.n = G;
                    for (int j = 0; j < G; ++j) { R.pos[j] = dv[j].pos; R.lp[j] = dv[j].lp; R.flags[j] = dv[j].flags; }
                    R.done = d.done; R.timeout = d.timeout; R.me = i; R.seq = seq; R.sync = flags_mode ? (one_device ? 1 : 2) : 0;
                    double* cp = (chain && flags_mode) ? d.chain + (size_t)it * W * D : (double*)nullptr;
                    double* cl = (chain && flags_mode) ? d.chain + chunk * (size_t)W * D + (size_t)it * W : (double*)nullptr;
                    if (nk <= 0) {
                        // (a context without rows in this half still has to tell the others that it is through)
                        if (flags_mode)
                            hipLaunchKernelGGL(vp::stretch_accept_block_kernel, dim3(1), dim3(thr), 0, c->stream, d.pos, d.lp, R, d.prop, d.lpnew,
                                               d.zz, D, s0, k0, 0, seed, step, h, d.nacc, d.nan, cp, cl);
                        continue;
                    }
                    const int split = stretch_split(c, half);      // (the choice vp_stretch_run makes for the whole half)
                    if (split >= 0) {
                        vp::StretchArgs sa{};
                        sa.pos = d.pos; sa.lp = d.lp; sa.nacc = d.nacc; sa.nanflag = d.nan;
                        sa.chain_pos = cp; sa.chain_lp = cl;
                        sa.a = a; sa.seed = seed; sa.step = step; sa.s0 = s0 + k0; sa.c0 = cc0; sa.nC = half; sa.half = h;
                        sa.rep = R;
                        launch_walker_stretch(c, nk, sa, c->stream, 0, split);    // (the form the WHOLE half would get)
                    } else {
                        hipLaunchKernelGGL(vp::stretch_propose_block_kernel, dim3((nk + thr - 1) / thr), dim3(thr), 0, c->stream, d.pos, D, s0,
                                           half, cc0, half, a, seed, step, h, k0, nk, d.prop, d.zz, R);
                        if ((rc = enqueue_lnprob(c, nk, d.prop, d.lpnew, c->stream, half))) return F.code(i, rc);
                        hipLaunchKernelGGL(vp::stretch_accept_block_kernel, dim3((nk + thr - 1) / thr), dim3(thr), 0, c->stream, d.pos, d.lp, R,
                                           d.prop, d.lpnew, d.zz, D, s0, k0, nk, seed, step, h, d.nacc, d.nan, cp, cl);
                    }
                    SLOT_TRY(F, i, hipGetLastError());
                }
                if (!flags_mode && (rc = multi_barrier(m))) return F.code(0, rc);
            }
            if (chain && !flags_mode) {
                SLOT_TRY(F, 0, hipSetDevice(c0->device));
                SLOT_TRY(F, 0, hipMemcpyAsync(dv[0].chain + (size_t)it * W * D, dv[0].pos, (size_t)W * D * sizeof(double), hipMemcpyDeviceToDevice, c0->stream));
                SLOT_TRY(F, 0, hipMemcpyAsync(dv[0].chain + chunk * (size_t)W * D + (size_t)it * W, dv[0].lp, (size_t)W * sizeof(double),
                                             hipMemcpyDeviceToDevice, c0->stream));
                // nobody writes into replica 0 (the next half-step's moved rows) before this snapshot is taken
                SLOT_TRY(F, 0, hipEventRecord(m->ev[0], c0->stream));
                for (int j = 1; j < G; ++j) {
                    vp_ctx* cj = m->ctx[j];
                    if (hipSetDevice(cj->device) != hipSuccess || hipStreamWaitEvent(cj->stream, m->ev[0], 0) != hipSuccess)
                        return F(j, VP_EHIP, "hipStreamWaitEvent failed");
                }
            }
        }
        if (chain && !flags_mode) {
            SLOT_TRY(F, 0, hipSetDevice(c0->device));
            SLOT_TRY(F, 0, hipMemcpyAsync(chain + (size_t)done * W * D, dv[0].chain, (size_t)n * W * D * sizeof(double), hipMemcpyDeviceToHost, c0->stream));
            SLOT_TRY(F, 0, hipMemcpyAsync(chain_lnprob + (size_t)done * W, dv[0].chain + chunk * (size_t)W * D, (size_t)n * W * sizeof(double),
                                         hipMemcpyDeviceToHost, c0->stream));
            SLOT_TRY(F, 0, hipStreamSynchronize(c0->stream));
        }
        if (chain && flags_mode) {
            // every context holds the chain rows of the walkers it moves (blocks k0 ... of both halves): merged here
            h_chunk.resize((size_t)n * row);
            for (int i = 0; i < G; ++i) {
                vp_ctx* c = m->ctx[i];
                const auto [k0, nk] = block_of(i, per, half);
                if (nk <= 0) continue;
                SLOT_TRY(F, i, hipSetDevice(c->device));
                SLOT_TRY(F, i, hipMemcpyAsync(h_chunk.data(), dv[i].chain, (size_t)n * W * D * sizeof(double), hipMemcpyDeviceToHost, c->stream));
                SLOT_TRY(F, i, hipMemcpyAsync(h_chunk.data() + (size_t)n * W * D, dv[i].chain + chunk * (size_t)W * D, (size_t)n * W * sizeof(double),
                                             hipMemcpyDeviceToHost, c->stream));
                SLOT_TRY(F, i, hipStreamSynchronize(c->stream));
                for (int t = 0; t < n; ++t)
                    for (int hh = 0; hh < 2; ++hh) {
                        const size_t w0 = (size_t)hh * half + k0;
                        std::memcpy(chain + ((size_t)(done + t) * W + w0) * D, h_chunk.data() + ((size_t)t * W + w0) * D, (size_t)nk * D * sizeof(double));
                        std::memcpy(chain_lnprob + (size_t)(done + t) * W + w0, h_chunk.data() + (size_t)n * W * D + (size_t)t * W + w0,
                                    (size_t)nk * sizeof(double));
                    }
            }
        }
        done += n;
    }
    // results: the ensemble from replica 0, every walker's acceptance count from the context that moved it, NaN flags from all
    int any_nan = 0, any_timeout = 0;
    std::vector<long long> h_nacc(W);
    for (int i = 0; i < G; ++i) {                      // (flags mode: replica 0 is complete only when every context is through)
        vp_ctx* c = m->ctx[i];
        SLOT_TRY(F, i, hipSetDevice(c->device));
        SLOT_TRY(F, i, hipStreamSynchronize(c->stream));
    }
    for (int i = 0; i < G; ++i) {
        vp_ctx* c = m->ctx[i];
        SLOT_TRY(F, i, hipSetDevice(c->device));
        int h_nan = 0, h_to = 0;
        SLOT_TRY(F, i, hipMemcpyAsync(&h_nan, dv[i].nan, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        SLOT_TRY(F, i, hipMemcpyAsync(&h_to, dv[i].timeout, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        SLOT_TRY(F, i, hipMemcpyAsync(h_nacc.data(), dv[i].nacc, (size_t)W * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        if (i == 0) {
            SLOT_TRY(F, i, hipMemcpyAsync(pos, dv[0].pos, (size_t)W * D * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            SLOT_TRY(F, i, hipMemcpyAsync(lnprob, dv[0].lp, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        }
        SLOT_TRY(F, i, hipStreamSynchronize(c->stream));
        any_nan |= h_nan; any_timeout |= h_to;
        if (naccepted) {
            const auto [k0, nk] = block_of(i, per, half);
            for (int hh = 0; hh < 2; ++hh)
                for (int k = k0; k < k0 + nk; ++k) naccepted[hh * half + k] += (int64_t)h_nacc[hh * half + k];
        }
    }
    if (any_timeout) return F(0, VP_ESTATE, "vp_multi_stretch_run: a context gave up waiting for its peers' half-step (in-kernel flags; try the multi_sync = 0 option)");
    if (any_nan) return F(0, VP_ENAN, "vp_multi_stretch_run: Probability function returned NaN");
    return VP_OK;
}

int vp_multi_slice_run(vp_multi* m, int W, int D, double* pos, double* lnprob, int have_lnprob, int nsteps, double* mu,
                       int* tune, double tolerance, int patience, int maxsteps, uint64_t seed, uint64_t step0,
                       double* chain, double* chain_lnprob, double* mu_history, int64_t* n_evals) {
    if (!m) return VP_EINVAL;
    std::lock_guard<std::mutex> g(m->mu);
    std::vector<std::unique_lock<std::mutex>> locks;
    if (int rc = multi_sampler_enter(m, "vp_multi_slice_run", W, D, pos, lnprob, locks)) return rc;
    const int G = (int)m->ctx.size();
    int bad = 0;
    const int rc = slice_run_impl(m, m->ctx.data(), G, W, D, pos, lnprob, have_lnprob, nsteps, mu, tune, tolerance, patience, maxsteps,
                                  seed, step0, chain, chain_lnprob, mu_history, n_evals, &bad);
    return rc ? multi_fail(m, bad, rc) : VP_OK;
}

void* vp_ctx_stream(const vp_ctx* c) { return c ? (void*)c->stream : nullptr; }

