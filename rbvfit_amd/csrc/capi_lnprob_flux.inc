// capi_lnprob_flux.inc -- entry points: vp_lnprob_batch (host buffers, completion by the output rows, pre-armed launches), model flux, row sums, components.
// A fragment of the ONE translation unit capi.hip (included there inside extern "C", in order; not a header of its own).
static int lnprob_host_begin(vp_ctx* c, int W, int D, const double* theta, int arm_next = 0) {
    int rc;
    const size_t tb = (size_t)W * D * sizeof(double), ob = (size_t)W * sizeof(double);
    // a launch waiting for exactly this shape of batch?  (anything else: it leaves before the workspace may move)
    bool use_armed = false;
    if (c->arm.live) {
        if (c->arm.W == W && arm_next >= 0 && prearm_eligible(c, W, tb) &&
            __atomic_load_n(&c->arm.h[vp::ARM_EXPIRED_WORD], __ATOMIC_ACQUIRE) != c->arm.seq)
            use_armed = true;
        else {
            if (__atomic_load_n(&c->arm.h[vp::ARM_EXPIRED_WORD], __ATOMIC_ACQUIRE) == c->arm.seq) {
                // it waited its whole budget for nothing -- the GPU was held for nobody: leave this caller alone for a while
                c->arm.live = false; ++c->arm.expired;
                c->arm.cooldown = c->arm.cooldown_next;
                c->arm.cooldown_next = std::min(4096, 2 * c->arm.cooldown_next);
                c->arm.used_streak = 0;
            }
            prearm_cancel(c);
        }
    }
    c->arm.inflight = false;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = ensure_workspace(c, W))) return rc;
    if ((rc = ensure_pinned(c, tb + ob))) return rc;
    if (!use_armed) std::memcpy(c->h_pinned, theta, tb);       // (a waiting launch gets theta pushed into its slots instead)
    double* h_out = c->h_pinned + (size_t)W * D;
    VP_HSTAMP(0);
    c->done_armed = false;
    c->sentinel_armed = false;
    // zerocopy_max defaults to 1 MiB; measured: 512 walkers x 6 parameters 50 us/call zero-copy vs 58 us with copies
    if (tb <= (size_t)std::max(0l, c->tune.zerocopy_max) && !c->tune.no_zerocopy) {
        // up to 1 MiB of theta: the kernels read theta from / write lnprob to the pinned (host-coherent)
        // buffer directly over PCIe -- no H2D/D2H copy commands on the latency path
        if (!c->h_pinned_dev) HIP_TRY(c, hipHostGetDevicePointer((void**)&c->h_pinned_dev, c->h_pinned, 0));
        double* dp = c->h_pinned_dev;
        // completion by the output rows themselves: every row is written exactly once per batch (out-of-bounds rows by the
        // launch that applies the prior, the others by the launch -- or the walker's last tile -- that finishes them)
        const bool poll_rows = c->tune.host_spin >= 2 && !c->sentinel_unsafe && !c->gather_rep && !carries_sentinel(theta, (size_t)W * D);
        if (use_armed && !poll_rows) { prearm_cancel(c); use_armed = false; std::memcpy(c->h_pinned, theta, tb); }
        if (poll_rows) {
            uint64_t* o = reinterpret_cast<uint64_t*>(h_out);
            for (int i = 0; i < W; ++i) o[i] = VP_SENTINEL_BITS;
            __atomic_thread_fence(__ATOMIC_RELEASE);
        }
        if (use_armed) {
            // the pattern rows are in place: push theta and the go words into the waiting launch's slots
            prearm_push(c, W, theta, vp::ARM_GO);
            c->arm.theta_src = theta;
            c->arm.live = false;
            c->arm.inflight = true;
            c->arm.cur = c->arm.live_stream;
            c->arm.seq_inflight = c->arm.seq;
            ++c->arm.used;
            if (++c->arm.used_streak >= 16) c->arm.cooldown_next = 8;
            record_launch(c, plan_lnprob(c, W), W);       // (a walker launch: prearm_eligible)
        } else {
            c->arm.cur = c->stream;
            if ((rc = enqueue_lnprob(c, W, dp, dp + (size_t)W * D, c->stream))) return rc;
        }
        if (poll_rows) {
            // the launch for the caller's NEXT batch of this shape, behind this one on the stream
            if (arm_next > 0 && prearm_eligible(c, W, tb) && (rc = prearm_launch(c, W))) return rc;
            c->sentinel_armed = true; c->sentinel_W = W; c->sentinel_out = h_out;
            VP_HSTAMP(1);
            return VP_OK;
        }
    } else {
        HIP_TRY(c, hipMemcpyAsync(c->d_theta, c->h_pinned, tb, hipMemcpyHostToDevice, c->stream));
        if ((rc = enqueue_lnprob(c, W, c->d_theta, c->d_out, c->stream))) return rc;
        HIP_TRY(c, hipMemcpyAsync(h_out, c->d_out, ob, hipMemcpyDeviceToHost, c->stream));
    }
    // completion word behind the batch (the command processor writes it once everything before it on the stream is done
    // and visible to the host); where the runtime refuses, host_wait falls back to hipStreamSynchronize
    if (c->tune.host_spin) {
        if (!c->h_done) {
            if (hipHostMalloc((void**)&c->h_done, 64, hipHostMallocMapped) != hipSuccess) { c->h_done = nullptr; (void)hipGetLastError(); }
            else *c->h_done = 0;
        }
        void* dptr = nullptr;
        if (c->h_done && hipHostGetDevicePointer(&dptr, c->h_done, 0) == hipSuccess &&
            hipStreamWriteValue32(c->stream, dptr, ++c->done_seq, 0) == hipSuccess)
            c->done_armed = true;
        else
            (void)hipGetLastError();
    }
    VP_HSTAMP(1);
    return VP_OK;
}
// wait for the batch lnprob_host_begin enqueued: spin on the completion word (no interrupt, no driver call on the way),
// hipStreamSynchronize when the word is not armed or has not come after 20 ms (a long batch: the interrupt is cheap then)
static int host_wait(vp_ctx* c) {
    if (c->sentinel_armed) {
        // rows land in any order; walk them once, waiting at the first one that is still the pattern
        c->sentinel_armed = false;
        const uint64_t* o = reinterpret_cast<const uint64_t*>(c->sentinel_out);
        const int W = c->sentinel_W;
        const auto t0 = std::chrono::steady_clock::now();
        int i = 0;
        // (a batch handed to a pre-armed launch: the launch may have given up waiting just as the rows and go words were on their way --
        //  it says so; some of its workgroups may have met their rows and run.  The batch is then started again the ordinary way:
        //  the launch armed behind it is sent away, the stream drains, the rows are set to the pattern again)
        auto relaunch = [&]() -> int {
            c->arm.inflight = false;
            prearm_cancel(c);
            HIP_TRY(c, hipSetDevice(c->device));
            // some workgroups of the expired launch may have met their rows and run: nothing of it may still write when the
            // rows are set to the pattern again
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            // (the split form counts a walker's workgroups in: groups of the expired launch that ran have left their tickets)
            if (c->d_ticket && c->capW > 0) HIP_TRY(c, hipMemset(c->d_ticket, 0, (size_t)c->capW * sizeof(unsigned int)));
            std::memcpy(c->h_pinned, c->arm.theta_src, (size_t)W * c->D * sizeof(double));
            uint64_t* orow = const_cast<uint64_t*>(o);
            for (int k = 0; k < W; ++k) orow[k] = VP_SENTINEL_BITS;
            __atomic_thread_fence(__ATOMIC_RELEASE);
            i = 0;
            c->arm.cur = c->stream;
            double* dp = c->h_pinned_dev;
            return enqueue_lnprob(c, W, dp, dp + (size_t)W * c->D, c->stream);
        };
        for (unsigned int spins = 0; i < W; ++spins) {
            while (i < W && __atomic_load_n(o + i, __ATOMIC_ACQUIRE) != VP_SENTINEL_BITS) {
#ifdef VP_STAMPS
                if (i == 0) VP_HSTAMP(2);
#endif
                ++i;
            }
            if (i == W) { VP_HSTAMP(3); if (c->arm.inflight) c->arm.misses = 0; return VP_OK; }
            __builtin_ia32_pause();
            if (c->arm.inflight && (spins & 63u) == 63u &&
                (__atomic_load_n(&c->arm.h[vp::ARM_EXPIRED_WORD], __ATOMIC_ACQUIRE) == c->arm.seq_inflight ||
                 __atomic_load_n(&c->arm.h[vp::ARM_STUCK_WORD], __ATOMIC_ACQUIRE) == c->arm.seq_inflight)) {      // (a workgroup gave up on its own: same cure)
                ++c->arm.expired; --c->arm.used;
                // (the go words were on their way and the launch still gave up: once is a caller that arrived at the last moment;
                //  three times in a row is a system where the pushes do not reach the launch in time -- no more pre-armed launches)
                if (++c->arm.misses >= 3) c->arm.bar = 0;
                int rc = relaunch();
                if (rc) return rc;
            }
            if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
        }
        if (i == W) return VP_OK;
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->arm.inflight && c->arm.cur ? c->arm.cur : c->stream));     // (a long batch: the interrupt is cheap then; everything is written behind it)
        if (c->arm.inflight) {
            // ... unless workgroups of a pre-armed launch left on their own (arm_wait's last resort): rows still carry the pattern
            bool missing = false;
            for (int k = 0; k < W; ++k) missing |= __atomic_load_n(o + k, __ATOMIC_ACQUIRE) == VP_SENTINEL_BITS;
            if (missing) {
                c->arm.bar = 0;
                int rc = relaunch();
                if (rc) return rc;
                HIP_TRY(c, hipStreamSynchronize(c->stream));
            }
        }
        return VP_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->done_armed) {
        const uint32_t want = c->done_seq;
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned int spins = 0;; ++spins) {
            if (__atomic_load_n(c->h_done, __ATOMIC_ACQUIRE) == want) { VP_HSTAMP(3); return VP_OK; }
            __builtin_ia32_pause();
            if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
        }
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return VP_OK;
}
static int lnprob_host_end(vp_ctx* c, int W, int D, double* out) {
    int rc;
    if ((rc = host_wait(c))) return rc;
    std::memcpy(out, c->h_pinned + (size_t)W * D, (size_t)W * sizeof(double));
    VP_HSTAMP(4);
    return VP_OK;
}

int vp_lnprob_batch(vp_ctx* c, int W, int D, const double* theta, double* out) {
    if (!c) return VP_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    int rc = check_batch_args(c, W, D, theta, out);
    if (rc) return rc;
    if (W == 0) return VP_OK;
#ifdef VP_STAMPS
    g_host_t0 = std::chrono::steady_clock::now();
#endif
    prearm_cancel_others(c);
    // pre-arm the next call's launch?  (prearm = -1: when this call came quickly behind the last one's return -- a sampler's loop)
    int arm_next = 0;
    if (c->tune.prearm > 0) arm_next = 1;
    else if (c->tune.prearm < 0 && c->arm.have_last && c->arm.last_W == W) {    // (ragged batches -- a slice sampler's rounds -- never arm)
        const double gap = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - c->arm.last_return).count();
        if (gap < 0.5 * std::max(1, c->tune.prearm_us)) {
            c->arm.gap_ema_us = c->arm.gap_ema_us > 0.0 ? 0.75 * c->arm.gap_ema_us + 0.25 * gap : gap;
            arm_next = 1;
        } else {
            c->arm.gap_ema_us = 0.0;             // a pause: the rhythm starts again
        }
        if (arm_next && c->arm.cooldown > 0) { --c->arm.cooldown; arm_next = 0; }
    }
    c->arm.last_W = W;
    if ((rc = lnprob_host_begin(c, W, D, theta, arm_next))) return rc;
    rc = lnprob_host_end(c, W, D, out);
    c->arm.inflight = false;
    c->arm.last_return = std::chrono::steady_clock::now();
    c->arm.have_last = true;
    return rc;
}
int vp_prearm_counts(vp_ctx* c, int64_t* used, int64_t* expired, int64_t* cancelled) {
    if (!c) return VP_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (used) *used = c->arm.used;
    if (expired) *expired = c->arm.expired;
    if (cancelled) *cancelled = c->arm.cancelled;
    return VP_OK;
}

// (called with c->mu held) prep + tile launches that write the (W, P) model flux of one instrument
static int enqueue_model_flux(vp_ctx* c, int inst, int W, const double* d_theta, double* d_out, int convolved, hipStream_t s) {
    int rc;
    if ((rc = ensure_workspace(c, W))) return rc;
    const Instrument& in = c->inst[inst];
    const bool gen = in.dev.method == VP_VOIGT_WOFZ;      // model_flux has no prior box: theta may be anything
    GenFlags gfl{nullptr, nullptr, nullptr, nullptr, 0};
    if (gen && (rc = genflag_acquire(c, W, s, &gfl))) return rc;
    const vp::FinalizeArgs nofin{};
    const int* gf = gfl.use;
    // far lines from the blocks' expansions, as in the lnprob launches (convolved flux; same rule for when the extra launch pays)
    LaunchPlan p;
    p.kind = -1;
    if (convolved && in.ff_on && c->d_ff && c->tune.flux_farfield != 0 &&
        (c->tune.flux_farfield > 0 || ff_pays(in.dev, ff_score(in, in.dev, W)))) p.ff_first = inst;
    record_launch(c, p, W);
    TileOpts o;
    o.ff = p.ff_first < 0 ? nullptr : c->d_ff;
    o.gen_slots = gfl.slots;
    // Batches the walker kernel takes as lnprob batches (one instrument, no cluster records, the workgroups fit the CUs): the rows in
    // ONE launch, workgroup = walker -- records formed in the workgroup, no record-preparation launch in front (C1 at 512 rows
    // 28 -> 24 us); walkers with a line outside the fast domain are left to the generic launch behind it, as in the tile path.
    if (convolved && !o.ff && inst == 0 && c->inst.size() == 1 && in.dev.NCm == 0 && c->tune.flux_walker != 0 && !c->profiling &&
        !c->gather_rep && walker_applies(c, W) && in.dev.method == VP_VOIGT_WOFZ) {
        vp::WalkerArgs a = walker_args(c, W, d_theta, d_out, 0.0);
        a.flux_stride = in.dev.P;
        a.genflag = gfl.use; a.genflag_clear = gfl.clear; a.gen_any = gfl.any; a.gen_any_clear = gfl.any_clear;
        vp::InstDev d0 = in.dev_w;
        vp::LinesDev t0 = in.lines;
        d0.NCm = 0; t0.NCm = 0;
        hipLaunchKernelGGL((vp::walker_kernel<0, false, false, false, 1>), dim3(W), dim3(64 * walker_tiles(c)), walker_lds_bytes(c), s, d0, t0, a,
                           vp::StretchArgs{});
        o.theta_rebuild = d_theta;
        o.D = c->D;
        launch_tile<1, true>(in, c->d_lc, nullptr, d_out, in.dev.P, 0, W, s, nofin, gf, o);
        HIP_TRY(c, hipGetLastError());
        return VP_OK;
    }
    launch_prep(c, in, d_theta, W, 0, nullptr, gfl, s);
    if (o.ff) launch_farfield(c, p, inst, o.ff, false, W, s);
    if (convolved) {
        launch_tile<1, false>(in, c->d_lc, nullptr, d_out, in.dev.P, 0, W, s, nofin, gf, o);
        if (gen) launch_tile<1, true>(in, c->d_lc, nullptr, d_out, in.dev.P, 0, W, s, nofin, gf, o);
    } else {
        launch_tile<2, false>(in, c->d_lc, nullptr, d_out, in.dev.P, 0, W, s, nofin, gf, o);
        if (gen) launch_tile<2, true>(in, c->d_lc, nullptr, d_out, in.dev.P, 0, W, s, nofin, gf, o);
    }
    HIP_TRY(c, hipGetLastError());
    return VP_OK;
}

int vp_model_flux_batch_device(vp_ctx* c, int inst, int W, int D, const double* d_theta, double* d_out, int convolved,
                               void* hip_stream) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    int rc = check_batch_args(c, W, D, d_theta, d_out);
    if (rc) return rc;
    if (inst < 0 || inst >= (int)c->inst.size()) return fail(c, VP_EINVAL, "vp_model_flux_batch: instrument index out of range");
    if (W == 0) return VP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if ((rc = foreign_stream_fence(c, s))) return rc;
    return enqueue_model_flux(c, inst, W, d_theta, d_out, convolved, s);
}

int vp_model_flux_batch(vp_ctx* c, int inst, int W, int D, const double* theta, double* out, int convolved) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);          // held from staging theta to the copy-back: d_theta / d_scratch are the context's
    int rc = check_batch_args(c, W, D, theta, out);
    if (rc) return rc;
    if (inst < 0 || inst >= (int)c->inst.size()) return fail(c, VP_EINVAL, "vp_model_flux_batch: instrument index out of range");
    if (W == 0) return VP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = ensure_workspace(c, W))) return rc;
    const size_t P = c->inst[inst].dev.P;
    if ((rc = ensure_scratch(c, (size_t)W * P * sizeof(double)))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_theta, theta, (size_t)W * D * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = enqueue_model_flux(c, inst, W, c->d_theta, c->d_scratch, convolved, c->stream))) return rc;
    HIP_TRY(c, hipMemcpyAsync(out, c->d_scratch, (size_t)W * P * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return VP_OK;
}

// out[w] = c0 - sum_p weights[p] * flux[w][p]: one workgroup per row, the lanes' partial sums added in a fixed order
namespace { __global__ __launch_bounds__(256) void row_weighted_sum_kernel(const double* __restrict__ rows, int P, const double* __restrict__ wts,
                                                                          double c0, double* __restrict__ out) {
    __shared__ double part[256];
    const double* __restrict__ r = rows + (size_t)blockIdx.x * P;
    double s = 0.0;
    for (int p = threadIdx.x; p < P; p += 256) s = __builtin_fma(wts[p], r[p], s);
    part[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = c0 - part[0];
} }

int vp_model_flux_rowsum(vp_ctx* c, int inst, int W, int D, const double* theta, const double* weights, double c0, int convolved, double* out) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    int rc = check_batch_args(c, W, D, theta, out);
    if (rc) return rc;
    if (inst < 0 || inst >= (int)c->inst.size()) return fail(c, VP_EINVAL, "vp_model_flux_rowsum: instrument index out of range");
    if (!weights) return fail(c, VP_EINVAL, "vp_model_flux_rowsum: NULL weights");
    if (W == 0) return VP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = ensure_workspace(c, W))) return rc;
    const size_t P = c->inst[inst].dev.P;
    struct Dev { double *rows, *w, *s; } d;       // scratch: the (W, P) rows | the P weights | the W sums
    if ((rc = carve_scratch(c, [&](Arena& A) { d = Dev{A.take<double>((size_t)W * P), A.take<double>(P), A.take<double>(W)}; }))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_theta, theta, (size_t)W * D * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d.w, weights, P * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = enqueue_model_flux(c, inst, W, c->d_theta, d.rows, convolved, c->stream))) return rc;
    hipLaunchKernelGGL(row_weighted_sum_kernel, dim3(W), dim3(256), 0, c->stream, d.rows, (int)P, d.w, c0, d.s);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, d.s, (size_t)W * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return VP_OK;
}

int vp_model_flux_components(vp_ctx* c, int inst, int W, int D, const double* theta, double* out) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    int rc = check_batch_args(c, W, D, theta, out);
    if (rc) return rc;
    if (inst < 0 || inst >= (int)c->inst.size()) return fail(c, VP_EINVAL, "vp_model_flux_components: instrument index out of range");
    if (W == 0) return VP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = ensure_workspace(c, W))) return rc;
    Instrument in = c->inst[inst];                 // local copy: line_sel = -2 makes the line a grid dimension
    in.allocs.clear();
    in.dev.line_sel = -2;
    const size_t P = in.dev.P, L = in.dev.L;
    // ONE launch per block of walkers evaluates all L per-line profiles (grid = walkers x tiles x lines) straight into
    // the (w, l, p) layout of `out`; blocks of at most ~1 GiB of output keep the device scratch bounded
    const size_t per_walker = L * P * sizeof(double);
    const int wblock = (int)std::max<size_t>(1, std::min<size_t>((size_t)W, ((size_t)1 << 30) / per_walker));
    if ((rc = ensure_scratch(c, (size_t)wblock * per_walker))) return rc;
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemcpyAsync(c->d_theta, theta, (size_t)W * D * sizeof(double), hipMemcpyHostToDevice, s));
    const bool gen = in.dev.method == VP_VOIGT_WOFZ;
    GenFlags gfl{nullptr, nullptr, nullptr, nullptr, 0};
    if (gen && (rc = genflag_acquire(c, W, s, &gfl))) return rc;
    launch_prep(c, in, c->d_theta, W, 0, nullptr, gfl, s);
    const vp::FinalizeArgs nofin{};
    const size_t nrec = (size_t)(in.dev.L + in.dev.NCm) * vp::LC_STRIDE;
    TileOpts o;
    o.grid_z = (int)L;
    o.gen_slots = gfl.slots;
    for (int w0 = 0; w0 < W; w0 += wblock) {
        const int nw = std::min(wblock, W - w0);
        const int* gf = gen ? gfl.use + w0 : (const int*)nullptr;
        launch_tile<2, false>(in, c->d_lc + (size_t)w0 * nrec, nullptr, c->d_scratch, (int)(L * P), 0, nw, s, nofin, gf, o);
        if (gen) launch_tile<2, true>(in, c->d_lc + (size_t)w0 * nrec, nullptr, c->d_scratch, (int)(L * P), 0, nw, s, nofin, gf, o);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(out + (size_t)w0 * L * P, c->d_scratch, (size_t)nw * per_walker, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    return VP_OK;
}

