// capi_setup.inc -- entry points: version, context life cycle, options, bounds, instruments, vp_lnprob_batch_device.
// A fragment of the ONE translation unit capi.hip (included there inside extern "C", in order; not a header of its own).

const char* vp_version(void) { return "rbvfit_amd " RBVFIT_AMD_VERSION " (gfx950, hip)"; }

int vp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* vp_last_error(const vp_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int vp_ctx_create(vp_ctx** out, int device_id) {
    if (!out) return fail(nullptr, VP_EINVAL, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, VP_EHIP, std::string("no usable HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
    if (device_id < 0 || device_id >= n) return fail(nullptr, VP_EINVAL, "device_id out of range");
    vp_ctx* c = new (std::nothrow) vp_ctx();
    if (!c) return fail(nullptr, VP_ENOMEM, "out of host memory");
    c->device = device_id;
    c->tune = tuning_from_env();
    if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
        std::string m = std::string("context creation failed: ") + hipGetErrorString(e);
        delete c;
        return fail(nullptr, VP_EHIP, m);
    }
    // Dynamic LDS a workgroup may ask for: the device's per-workgroup limit (160 KiB on MI355X).  The
    // tile and walker kernels are told they may use all of it (a no-op where the runtime does not need it).
    int lds_max = 0;
    if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device_id) == hipSuccess && lds_max > 0)
        c->lds_limit = (size_t)lds_max;
    for (const void* f : {(const void*)vp::walker_kernel<0, false, false>, (const void*)vp::walker_kernel<0, true, false>,
                          (const void*)vp::walker_kernel<1, false, false>, (const void*)vp::walker_kernel<0, false, true>,
                          (const void*)vp::walker_kernel<1, false, true>,
                          (const void*)vp::walker_kernel<0, false, false, true>, (const void*)vp::walker_kernel<1, false, false, true>,
                          (const void*)vp::walker_kernel<0, true, false, true>, (const void*)vp::walker_kernel<0, false, false, false, 1>,
                          (const void*)vp::walker_kernel<0, false, false, false, 0, true>, (const void*)vp::walker_kernel<1, false, false, false, 0, true>,
                          (const void*)vp::walker_kernel<0, false, true, false, 0, true>, (const void*)vp::walker_kernel<1, false, true, false, 0, true>,
                          (const void*)vp::walker_kernel<0, false, false, true, 0, true>, (const void*)vp::walker_kernel<1, false, false, true, 0, true>,
                          (const void*)vp::walker_kernel2<0, false, true>, (const void*)vp::walker_kernel2<1, false, true>,
                          (const void*)vp::walker_kernel4<0, false, true>, (const void*)vp::walker_kernel4<1, false, true>,
                          (const void*)vp::tile_kernel1<0, true>, (const void*)vp::tile_kernel1<0, false>, (const void*)vp::tile_kernel1<1, false>,
                          (const void*)vp::tile_generic_kernel<0, false>, (const void*)vp::tile_generic_kernel<1, false>, (const void*)vp::tile_generic_kernel<1, true>,
                          (const void*)vp::tile_generic_kernel<2, false>, (const void*)vp::tile_kernel<0, 1, false, true>,
                          (const void*)vp::walker_kernel2<0, false>, (const void*)vp::walker_kernel2<0, true>,
                          (const void*)vp::walker_kernel2<1, false>, (const void*)vp::walker_kernel2<1, true>,
                          (const void*)vp::walker_kernel4<0, false>, (const void*)vp::walker_kernel4<0, true>,
                          (const void*)vp::walker_kernel4<1, false>, (const void*)vp::walker_kernel4<1, true>,
                          (const void*)vp::tile_kernel<0, 0, false, true>, (const void*)vp::tile_kernel_multi<0>, (const void*)vp::tile_kernel_multi<1>,
                          (const void*)vp::tile_kernel<0, 0, false>, (const void*)vp::tile_kernel<0, 1, false>, (const void*)vp::tile_kernel<0, 2, false>,
                          (const void*)vp::tile_kernel<1, 0, false>, (const void*)vp::tile_kernel<1, 1, false>,
                          (const void*)vp::tile_kernel<1, 2, false>})
        (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_limit);
    (void)hipGetLastError();
    ctx_register(c);
    *out = c;
    return VP_OK;
}

int vp_set_option(vp_ctx* c, const char* name, long value) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    if (!name) return fail(c, VP_EINVAL, "vp_set_option: NULL name");
    for (const Knob& k : g_knobs)
        if (std::strcmp(k.name, name) == 0) {
            set_knob(c->tune, k, value);
            return VP_OK;
        }
    return fail(c, VP_EINVAL, std::string("vp_set_option: unknown option '") + name + "'");
}

static void gather_release(vp_ctx* c) {
    vp_ctx::Gather& g = c->gather;
    for (int r = 0; r < g.world && r < vp::MAX_REPLICAS; ++r) {
        if (r == g.rank) continue;
        if (g.local_peers) continue;           // (plain pointers into contexts of this process: theirs to free)
        if (g.peer_buf[r]) (void)hipIpcCloseMemHandle(g.peer_buf[r]);
        if (g.peer_flags[r]) (void)hipIpcCloseMemHandle(g.peer_flags[r]);
    }
    if (g.buf) (void)hipFree(g.buf);
    if (g.flags) (void)hipFree(g.flags);
    if (g.done) (void)hipFree(g.done);
    (void)hipGetLastError();
    g = vp_ctx::Gather{};
}

int vp_ctx_destroy(vp_ctx* c) {
    if (!c) return VP_OK;
    ctx_unregister(c);
    { std::lock_guard<std::mutex> g(c->mu); prearm_cancel(c); }
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    if (c->arm.h) hipHostFree(c->arm.h);
    if (c->arm.ev) hipEventDestroy(c->arm.ev);
    if (c->arm.slots) hipFree(c->arm.slots);
    if (c->h_gen_any) hipHostFree(c->h_gen_any);
    for (auto& in : c->inst) for (void* p : in.allocs) hipFree(p);
    for (void* p : {(void*)c->d_lb, (void*)c->d_ub, (void*)c->d_theta, (void*)c->d_out, (void*)c->d_lc, (void*)c->d_partial,
                    (void*)c->d_flags, (void*)c->d_ticket, (void*)c->d_genflag, (void*)c->d_tile_off, (void*)c->d_sum_logw, (void*)c->d_scratch,
                    (void*)c->d_ff, (void*)c->grad.fl, (void*)c->grad.q, (void*)c->grad.rec, (void*)c->grad.part, (void*)c->grad.io,
                    (void*)c->fisher.g, (void*)c->fisher.J, (void*)c->fisher.part, (void*)c->fisher.io})
        if (p) hipFree(p);
    if (c->h_pinned) hipHostFree(c->h_pinned);
    if (c->h_done) hipHostFree(c->h_done);
    gather_release(c);
    for (hipEvent_t e : c->ev_pool) hipEventDestroy(e);
    if (c->ev_fork) hipEventDestroy(c->ev_fork);
    if (c->ev_join) hipEventDestroy(c->ev_join);
    if (c->stream2) hipStreamDestroy(c->stream2);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
    return VP_OK;
}

int vp_set_bounds(vp_ctx* c, int D, const double* lb, const double* ub) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    if (c->h_gen_any) c->h_gen_any[0] = 0;          // (new prior box: nothing known about walkers outside the fast domain)
    if (D <= 0 || !lb || !ub) return fail(c, VP_EINVAL, "vp_set_bounds: D must be positive and lb/ub non-NULL");
    if (!c->inst.empty() && D != c->D) return fail(c, VP_ESTATE, "vp_set_bounds: D differs from the D the instruments were validated against");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize());
    if (c->d_lb) HIP_TRY(c, hipFree(c->d_lb));
    if (c->d_ub) HIP_TRY(c, hipFree(c->d_ub));
    c->d_lb = c->d_ub = nullptr;
    int rc;
    if ((rc = upload<double>(c, nullptr, lb, D, &c->d_lb))) return rc;
    if ((rc = upload<double>(c, nullptr, ub, D, &c->d_ub))) return rc;
    if (D != c->D) {   // drop the workspace, it is resized lazily
        for (void* p : {(void*)c->d_theta, (void*)c->d_out, (void*)c->d_lc, (void*)c->d_partial, (void*)c->d_flags})
            if (p) hipFree(p);
        c->d_theta = c->d_out = c->d_lc = c->d_partial = nullptr; c->d_flags = nullptr; c->capW = 0;
    }
    c->D = D;
    if (carries_sentinel(lb, D) || carries_sentinel(ub, D)) c->sentinel_unsafe = true;
    c->h_lb.assign(lb, lb + D);
    c->h_ub.assign(ub, ub + D);
    for (auto& in : c->inst) analyse_generic(c, in);
    return VP_OK;
}

int vp_add_instrument(vp_ctx* c, int P, const double* wave, const double* flux, const double* inv_sigma2,
                      const double* log_inv_sigma2, int L, const double* lambda0, const double* gamma,
                      const double* f, const double* zfac, const int32_t* N_idx, const int32_t* b_idx,
                      const int32_t* v_idx, int K, const double* taps, int lsf_mode, int voigt_method,
                      int* inst_index) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    if (c->h_gen_any) c->h_gen_any[0] = 0;
    if (c->D <= 0) return fail(c, VP_ESTATE, "vp_add_instrument: call vp_set_bounds first (theta indices are validated against D)");
    if (P <= 0 || !wave || !flux || !inv_sigma2 || !log_inv_sigma2) return fail(c, VP_EINVAL, "vp_add_instrument: empty or NULL spectrum");
    if (L <= 0 || !lambda0 || !gamma || !f || !zfac || !N_idx || !b_idx || !v_idx) return fail(c, VP_EINVAL, "vp_add_instrument: empty or NULL line tables");
    if (voigt_method != VP_VOIGT_WOFZ && voigt_method != VP_VOIGT_FAST) return fail(c, VP_EINVAL, "vp_add_instrument: unknown voigt_method");
    if (lsf_mode < VP_LSF_NONE || lsf_mode > VP_LSF_ASTROPY_EXTEND) return fail(c, VP_EINVAL, "vp_add_instrument: unknown lsf_mode");
    if (lsf_mode != VP_LSF_NONE && (K <= 0 || !taps)) return fail(c, VP_EINVAL, "vp_add_instrument: lsf_mode set but no taps");
    if (lsf_mode != VP_LSF_NONE && (K % 2) == 0) return fail(c, VP_EINVAL, "vp_add_instrument: the number of taps must be odd");
    if (K > 2049) return fail(c, VP_EINVAL, "vp_add_instrument: more than 2049 LSF taps is not supported");
    if (L > 4096) return fail(c, VP_EINVAL, "vp_add_instrument: more than 4096 lines per instrument is not supported");
    for (int l = 0; l < L; ++l) {
        if (N_idx[l] < 0 || N_idx[l] >= c->D || b_idx[l] < 0 || b_idx[l] >= c->D || v_idx[l] < 0 || v_idx[l] >= c->D)
            return fail(c, VP_EINVAL, "vp_add_instrument: theta index of line " + std::to_string(l) + " outside [0, D)");
    }
    if (carries_sentinel(wave, P) || carries_sentinel(flux, P) || carries_sentinel(inv_sigma2, P) || carries_sentinel(lambda0, L) ||
        carries_sentinel(gamma, L) || carries_sentinel(f, L) || carries_sentinel(zfac, L) || (taps && K > 0 && carries_sentinel(taps, K)))
        c->sentinel_unsafe = true;
    HIP_TRY(c, hipSetDevice(c->device));
    Instrument in;
    int rc;
    // flipped (and, for the astropy branch, normalised) taps: out[p] = sum_j kflip[j] f[p - halo_lo + j]
    std::vector<double> kflip;
    int Kuse = 1, cidx = 0;
    if (lsf_mode == VP_LSF_NONE) {
        kflip.assign(1, 1.0);
    } else {
        Kuse = K; cidx = K / 2;
        double norm = 1.0;
        if (lsf_mode == VP_LSF_ASTROPY_EXTEND) { norm = 0.0; for (int j = 0; j < K; ++j) norm += taps[j]; }
        kflip.resize(K);
        for (int j = 0; j < K; ++j) {
            double t = taps[K - 1 - j];
            kflip[j] = (lsf_mode == VP_LSF_ASTROPY_EXTEND) ? t / norm : t;
        }
    }
    std::vector<double> ginv(P);
    for (int p = 0; p < P; ++p) ginv[p] = 1.0 / wave[p];
    double *d_wave, *d_ginv, *d_flux, *d_w, *d_k, *d_l0, *d_g, *d_f, *d_z, *d_fr0;
    std::vector<double> freq0(L);
    for (int l = 0; l < L; ++l) freq0[l] = vp::C_FREQ / lambda0[l];     // voigt_model.py:143
    int *d_n, *d_b, *d_v;
#define UP(T, h, n, d) if ((rc = upload<T>(c, &in, h, n, &d))) { for (void* p : in.allocs) hipFree(p); return rc; }
    UP(double, wave, P, d_wave) UP(double, ginv.data(), P, d_ginv)
    if ((rc = upload<double>(c, &in, flux, P, &d_flux, vp::OBS_PAD)) || (rc = upload<double>(c, &in, inv_sigma2, P, &d_w, vp::OBS_PAD))) {
        for (void* p : in.allocs) hipFree(p);
        return rc;
    }
    kflip.resize((kflip.size() + 7) & ~(size_t)7, 0.0);       // zero-padded to whole groups of 8 (what the LSF loop reads)
    UP(double, kflip.data(), kflip.size(), d_k)
    UP(double, lambda0, L, d_l0) UP(double, freq0.data(), L, d_fr0) UP(double, gamma, L, d_g) UP(double, f, L, d_f) UP(double, zfac, L, d_z)
    UP(int, N_idx, L, d_n) UP(int, b_idx, L, d_b) UP(int, v_idx, L, d_v)
    in.d_flux = d_flux; in.d_w = d_w;
    // multipole clusters: maximal runs of >= 3 (and <= 64) consecutive lines with the same rest
    // wavelength and redshift factor = the components of one transition (voigt_model.py:391-401)
    std::vector<int> cl_mp(L, -1), cl_end(L, 0), cl_first, cl_count;
    for (int l = 0; l < L;) {
        int e = l + 1;
        while (e < L && lambda0[e] == lambda0[l] && zfac[e] == zfac[l]) ++e;
        for (int k = l; k < e; ++k) cl_end[k] = e;
        const bool enable = !c->tune.no_multipole;
        if (enable && e - l >= c->tune.multipole_min && e - l <= 64 && voigt_method == VP_VOIGT_WOFZ) {
            cl_mp[l] = (int)cl_first.size();
            cl_first.push_back(l);
            cl_count.push_back(e - l);
        }
        l = e;
    }
    const int NCm = (int)cl_first.size();
    for (int k = 0; k < NCm; ++k)
        for (int l = cl_first[k]; l < cl_first[k] + cl_count[k] && l < 128; ++l) in.member_mask[l >> 6] |= 1ull << (l & 63);
    int *d_clmp, *d_clend, *d_clfirst, *d_clcount;
    UP(int, cl_mp.data(), L, d_clmp) UP(int, cl_end.data(), L, d_clend)
    UP(int, cl_first.data(), cl_first.size(), d_clfirst) UP(int, cl_count.data(), cl_count.size(), d_clcount)
    std::vector<int4> mem_info;                      // per member of a cluster: cluster, line, first member, member count
    for (int k = 0; k < NCm; ++k) {
        const int m0 = (int)mem_info.size();
        for (int j = 0; j < cl_count[k]; ++j) mem_info.push_back(int4{k, cl_first[k] + j, m0, cl_count[k]});
    }
    int4* d_meminfo;
    UP(int4, mem_info.data(), mem_info.size(), d_meminfo)
    in.lines = vp::LinesDev{L, d_l0, d_fr0, d_g, d_f, d_z, d_n, d_b, d_v, NCm, d_clfirst, d_clcount, d_clmp, d_clend,
                            (int)mem_info.size(), d_meminfo};
    vp::InstDev& d = in.dev;
    d.P = P; d.L = L; d.K = Kuse; d.halo_lo = Kuse - 1 - cidx; d.method = voigt_method; d.line_sel = -1;
    d.NCm = NCm;
#undef UP
    // Tile geometry: one wave evaluates 2*RB chunks of 64 consecutive pixels (RB register-blocked per pass);
    // a workgroup is 1, 2 or 4 such waves.  Single-wave workgroups need no cross-wave barrier and
    // let the hardware balance the walkers' tiles; longer LSFs take wider tiles to keep the halo
    // (K-1 re-evaluated pixels per tile) a small fraction.
    int nwaves = Kuse <= 33 ? 1 : Kuse <= 65 ? 2 : 4;
    int span = 2 * 64 * vp::RB * nwaves;                 // two register-blocked passes per wave
    if (c->tune.waves > 0) nwaves = std::min(4, c->tune.waves) == 3 ? 2 : std::min(4, c->tune.waves);   // tuning experiments: 1, 2 or 4
    if (c->tune.span > 0) span = std::max(64, (c->tune.span / 64) * 64);                         // (multiple of 64)
    if (Kuse > 257) { span = std::min(8192, ((4 * Kuse + 63) / 64) * 64); nwaves = 4; }
    const int need = P + Kuse - 1;
    if (need < span) span = std::max(64, ((need + 63) / 64) * 64);
    in.nwaves = nwaves;
    d.span = span; d.TP = span - (Kuse - 1);
    d.ntiles = (P + d.TP - 1) / d.TP;
    d.wave = d_wave; d.ginv = d_ginv; d.flux = d_flux; d.w = d_w; d.kflip = d_k;
    d.rbot = nullptr;
    {
        // NaN wavelength samples make NaN model pixels.  The reference's Gaussian branch (scipy convolve1d) lets each poison the K
        // outputs around it; its CustomKernel branch (astropy convolve, nan_treatment='interpolate': voigt_model.py:227,230) leaves
        // them out and divides every output by the kernel weight of the samples it did use.  The pattern is static, so the
        // reciprocal of that weight is a per-pixel table (taps in the order the device applies them; a window of NaNs only: NaN).
        bool any_nan = false;
        for (int p = 0; p < P; ++p) any_nan |= wave[p] != wave[p];
        if (any_nan) {
            // (the other branches -- scipy's convolve1d, no LSF -- get the same instances with a table of 1 and NaN: a NaN sample
            //  poisons exactly the outputs whose K taps reach it.  Left to the arithmetic it would also poison the outputs the
            //  ZERO taps of the padded tap groups reach, 0 x NaN being NaN)
            std::vector<double> rbot(P);
            const int halo = d.halo_lo;
            for (int p = 0; p < P; ++p) {
                double bot = 0.0;
                bool hit = false;
                for (int j = 0; j < Kuse; ++j) {
                    const int q = std::min(std::max(p - halo + j, 0), P - 1);
                    if (wave[q] == wave[q]) bot += kflip[j]; else hit = true;
                }
                if (lsf_mode == VP_LSF_ASTROPY_EXTEND) rbot[p] = bot != 0.0 ? 1.0 / bot : std::nan("");
                else rbot[p] = hit ? std::nan("") : 1.0;
            }
            double* d_rbot;
            if ((rc = upload<double>(c, &in, rbot.data(), rbot.size(), &d_rbot))) { for (void* q : in.allocs) hipFree(q); return rc; }
            d.rbot = d_rbot;
            in.nanfix = true;
        }
    }
    d.core_hint = nullptr;                               // (per geometry, below)
    d.ff_tab = nullptr; d.ff = nullptr; d.ff_nblk = 0; d.ff_members = 0;
    in.dev_s = d;                                        // one-pass tiles for small batches (same LDS layout rules)
    {
        const int span_s = 64 * vp::RB * nwaves;
        if (span_s < d.span && span_s - (Kuse - 1) >= 64) {
            in.dev_s.span = span_s; in.dev_s.TP = span_s - (Kuse - 1);
            in.dev_s.ntiles = (P + in.dev_s.TP - 1) / in.dev_s.TP;
        }
    }
    // far-field expansions: per block of 64 RB evaluated pixels the centre and half-width of 1/wave (both geometries)
    in.ff_on = voigt_method == VP_VOIGT_WOFZ && L <= 128 && (c->tune.farfield > 0 || (c->tune.farfield < 0 && L >= 8)) && !in.nanfix;
    if (in.ff_on) {
        for (vp::InstDev* gd : {&in.dev, &in.dev_s}) {
            const int blk_px = 64 * vp::RB, nblk = (gd->span + blk_px - 1) / blk_px;
            std::vector<double> tab((size_t)gd->ntiles * nblk * 4, 0.0);
            for (int t = 0; t < gd->ntiles; ++t) {
                const int p0 = t * gd->TP, nout = std::min(p0 + gd->TP, P) - p0, n_eval = nout + Kuse - 1, q0 = p0 - gd->halo_lo;
                for (int b = 0; b < nblk; ++b) {
                    double* e = tab.data() + ((size_t)t * nblk + b) * 4;
                    const int i0 = b * blk_px;
                    if (i0 >= n_eval) { e[0] = 0.0; e[1] = -1.0; e[2] = 0.0; e[3] = 0.0; continue; }
                    const int i1 = std::min(i0 + blk_px, n_eval) - 1;
                    const int qa = std::min(std::max(q0 + i0, 0), P - 1), qb = std::min(std::max(q0 + i1, 0), P - 1);
                    double gmin = ginv[qa], gmax = ginv[qa];
                    for (int q = qa; q <= qb; ++q) { gmin = std::min(gmin, ginv[q]); gmax = std::max(gmax, ginv[q]); }
                    const double gc = 0.5 * (gmax + gmin), hw = 0.5 * (gmax - gmin);
                    e[0] = gc; e[1] = hw; e[2] = hw > 0.0 ? 1.0 / hw : 0.0; e[3] = gc * e[2];
                    if (!(hw >= 0.0) || !(std::fabs(gc) <= 1.79e308)) { e[1] = -1.0; e[2] = 0.0; e[3] = 0.0; }   // NaN pixels: no expansion
                }
            }
            double* d_tab;
            if ((rc = upload<double>(c, &in, tab.data(), tab.size(), &d_tab))) { for (void* p : in.allocs) hipFree(p); return rc; }
            gd->ff_tab = d_tab; gd->ff_nblk = nblk; gd->ff = nullptr;
            if (gd == &in.dev) {
                // how much of the instrument the expansions will cover, estimated for Doppler widths at the geometric
                // centre of their bounds and lines at rest in their systems: the acceptance rule of farfield_kernel in
                // velocity units (block half-width <= distance / 8, nearest pixel >= 30 Doppler widths away)
                const double ckms = 299792.458;
                long cov = 0, tot = 0;
                for (size_t bk = 0; bk < tab.size() / 4; ++bk) {
                    const double gc = tab[4 * bk], hw = tab[4 * bk + 1];
                    if (!(hw >= 0.0) || !(gc > 0.0)) continue;
                    const double hwv = ckms * hw / gc;
                    for (int l = 0; l < L; ++l) {
                        const double lam = lambda0[l] * zfac[l];
                        double bl = c->h_lb[b_idx[l]], bu = c->h_ub.size() == c->h_lb.size() ? c->h_ub[b_idx[l]] : bl;
                        const double beff = (bl > 0.0 && bu > 0.0) ? std::sqrt(bl * bu) : 20.0;
                        const double dv = ckms * std::fabs(std::log(1.0 / (gc * lam)));
                        ++tot;
                        if (hwv <= dv / 8.0 && dv - hwv >= 30.0 * beff) ++cov;
                    }
                }
                in.ff_cover = tot > 0 ? (double)cov / (double)tot : 0.0;
                {
                    // members of near clusters line by line (farfield_kernel): only where a block is narrow against the
                    // lines -- half-width <= 1/8 of a distance of ~30 Doppler widths of the narrowest line allowed
                    std::vector<double> hwvs;
                    for (size_t bk = 0; bk < tab.size() / 4; ++bk)
                        if (tab[4 * bk + 1] >= 0.0 && tab[4 * bk] > 0.0) hwvs.push_back(ckms * tab[4 * bk + 1] / tab[4 * bk]);
                    double bmin = 1e300;
                    for (int l = 0; l < L; ++l) {
                        const double bl = c->h_lb[b_idx[l]], bu = c->h_ub.size() == c->h_lb.size() ? c->h_ub[b_idx[l]] : bl;
                        bmin = std::min(bmin, (bl > 0.0 && bu > 0.0) ? std::sqrt(bl * bu) : 20.0);
                    }
                    int members = 0;
                    if (!hwvs.empty() && NCm > 0 && !c->tune.no_ff_members) {
                        std::nth_element(hwvs.begin(), hwvs.begin() + hwvs.size() / 2, hwvs.end());
                        members = hwvs[hwvs.size() / 2] <= (30.0 / 8.0) * bmin ? 1 : 0;
                    }
                    in.dev.ff_members = members;
                }
                {
                    int members = 0;
                    for (size_t k = 0; k < cl_count.size(); ++k) members += cl_count[k];
                    in.ff_items = (int)cl_count.size() + (L - members);
                }
                if (getenv("RBVFIT_AMD_VERBOSE")) fprintf(stderr, "[rbvfit_amd] instrument %zu: far-field cover estimate %.3f (%d lines, %zu blocks)\n",
                                                          c->inst.size(), in.ff_cover, L, tab.size() / 4);
            }
        }
    }
    in.dev_s.ff_members = in.dev.ff_members;
    in.lds_bytes = (size_t)(span + vp::FL_PAD + 4 + vp::DAW_LDS_DOUBLES + vp::EXP_LDS_DOUBLES + (span / 64) * ((L + 63) / 64)) * sizeof(double);
    {
        in.dev_w = in.dev;
        in.lds_w = in.lds_bytes;
        if (in.nwaves != 1) {
            const int span_w = 2 * 64 * vp::RB;
            if (span_w - (Kuse - 1) >= 64 && c->tune.span == 0) {
                in.dev_w.span = span_w; in.dev_w.TP = span_w - (Kuse - 1);
                in.dev_w.ntiles = (P + in.dev_w.TP - 1) / in.dev_w.TP;
                in.dev_w.ff_tab = nullptr; in.dev_w.ff_nblk = 0;
                in.lds_w = (size_t)(span_w + vp::FL_PAD + 4 + vp::DAW_LDS_DOUBLES + vp::EXP_LDS_DOUBLES + (span_w / 64) * ((L + 63) / 64)) * sizeof(double);
            } else {
                in.lds_w = 0;
            }
        }
    }
    // walker_kernel's split form runs on the ONE-pass geometry of single-wave tiles (dev_s), with hints of its own
    if (in.nwaves == 1 && in.dev_s.span < in.dev.span && in.dev_s.ntiles >= 2 && c->tune.span == 0) {
        in.lds_s = (size_t)(in.dev_s.span + vp::FL_PAD + 4 + vp::DAW_LDS_DOUBLES + vp::EXP_LDS_DOUBLES + (in.dev_s.span / 64) * ((L + 63) / 64)) * sizeof(double);
        std::vector<int> zeros(std::max(in.dev_s.ntiles, vp::TILE_ORDER_AT), 0);
        if ((rc = upload<int>(c, &in, zeros.data(), zeros.size(), &in.split_hint))) { for (void* p : in.allocs) hipFree(p); return rc; }
    }
    if (in.lds_bytes + (size_t)std::max(0l, c->tune.lds_pad) > c->lds_limit) {
        for (void* p : in.allocs) hipFree(p);
        return fail(c, VP_EINVAL, "vp_add_instrument: a " + std::to_string(Kuse) + "-tap LSF with " + std::to_string(L) +
                    " lines needs " + std::to_string(in.lds_bytes) + " B of LDS per tile workgroup, the device allows " +
                    std::to_string(c->lds_limit));
    }
    in.sum_logw = neumaier_sum(log_inv_sigma2, P);
    // Per geometry: walker_kernel's hints (zero), then the order in which tile_kernel hands out the tiles -- by estimated
    // cost, the most expensive first, so that a launch ends on cheap workgroups wherever the lines sit on the grid: cost =
    // the tile's pixels within +-300 km/s of a line centre (at v = 0), summed over the lines (where the line-core and
    // near-wing tiers run); ties, and grids without lines, keep the grid order.
    {
        std::vector<int> core_lo(L, 1), core_hi(L, 0);
        if (P > 1 && wave[P - 1] > wave[0] && c->tune.tile_lpt) {
            for (int l = 0; l < L; ++l) {
                const double wc = lambda0[l] * zfac[l], hw = wc * (300.0 / 299792.458);
                const int lo = (int)(std::lower_bound(wave, wave + P, wc - hw) - wave);
                const int hi = (int)(std::upper_bound(wave, wave + P, wc + hw) - wave) - 1;
                if (hi >= lo) { core_lo[l] = lo; core_hi[l] = hi; }
            }
        }
        vp::InstDev* geoms[3] = {&in.dev, &in.dev_s, &in.dev_w};
        for (int gi = 0; gi < 3; ++gi) {
            vp::InstDev* gd = geoms[gi];
            bool reused = false;
            for (int gj = 0; gj < gi && !reused; ++gj)
                if (geoms[gj]->TP == gd->TP && geoms[gj]->ntiles == gd->ntiles) { gd->core_hint = geoms[gj]->core_hint; reused = true; }
            if (reused) continue;
            std::vector<int> tabl(vp::TILE_ORDER_AT + gd->ntiles, 0);
            std::vector<long> cost(gd->ntiles, 0);
            bool any = false;
            for (int l = 0; l < L; ++l)
                for (int t = core_lo[l] / gd->TP; core_hi[l] >= core_lo[l] && t <= std::min(gd->ntiles - 1, core_hi[l] / gd->TP); ++t) {
                    cost[t] += std::min(core_hi[l], (t + 1) * gd->TP - 1) - std::max(core_lo[l], t * gd->TP) + 1;
                    any = true;
                }
            if (any && gd->ntiles > 1) {
                std::vector<int> idx(gd->ntiles);
                for (int t = 0; t < gd->ntiles; ++t) idx[t] = t;
                std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return cost[a] > cost[b]; });
                for (int t = 0; t < gd->ntiles; ++t) tabl[vp::TILE_ORDER_AT + t] = idx[t] + 1;
            }
            // walker_kernel's deal of the tiles to its waves by that cost (WalkerArgs::wperm): waves k, k + 4, k + 8 of a workgroup
            // share a SIMD, so the tiles go out in tiers of four, every other tier backwards -- each SIMD one tile of every tier --,
            // starting behind the waves that form the records (they get the cheapest tiles).  Measured on C1, us per pass, tile
            // order / dealt: 256 walkers 15.98 / 15.68; 512 walkers (two workgroups per CU) 21.5 / 21.9 -- there two waves with
            // line cores that share a SIMD keep it issuing between them, so the deal is used for single-layer batches only
            if ((gd == &in.dev_w || (gi < 2 && in.dev_w.TP == gd->TP && in.dev_w.ntiles == gd->ntiles)) && gd->ntiles <= 16) {
                const int nw = gd->ntiles, ntask = std::min(nw, 1 + (L + 3) / 4);
                std::vector<int> idx(nw), seq(nw);
                for (int t = 0; t < nw; ++t) idx[t] = t;
                if (any) std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return cost[a] > cost[b]; });
                for (int k = 0; k < nw; ++k) seq[k] = (ntask + k) % nw;       // the waves with entry tasks come last (cheapest tiles)
                unsigned long long perm = 0xFEDCBA9876543210ull;
                for (int k = 0; k < nw; ++k) {
                    const int tier = k / 4, lo = tier * 4, hi = std::min(nw, lo + 4) - 1;
                    const int tile = idx[(tier & 1) ? hi - (k - lo) : k];
                    perm = (perm & ~(15ull << (4 * seq[k]))) | ((unsigned long long)tile << (4 * seq[k]));
                }
                in.wperm = perm;
                // ... and the deal for batches that put two workgroups on a CU (Instrument::wperm_shared, walker_deal_for): the tiles stay
                // in grid order inside three groups -- the cheapest tiles on the waves with entry tasks, then the tiles with line
                // cores (more than half the largest cost: one per SIMD where there are four), then the rest.  Measured on C1 at 512
                // walkers, us per pass (profiles/simd_deal_notes.md): grid order 21.20, the deal above 21.67, this one 20.80.
                {
                    long cmax = 0;
                    for (int t = 0; t < nw; ++t) cmax = std::max(cmax, cost[t]);
                    std::vector<int> asc(nw);
                    for (int t = 0; t < nw; ++t) asc[t] = t;
                    std::stable_sort(asc.begin(), asc.end(), [&](int a, int b) { return cost[a] < cost[b]; });     // cheapest first, ties in grid order
                    std::vector<int> grp(nw, 2);
                    for (int t = 0; t < nw; ++t) if (cmax > 0 && 2 * cost[t] > cmax) grp[t] = 1;
                    for (int k = 0; k < ntask; ++k) grp[asc[k]] = 0;
                    unsigned long long ps = 0xFEDCBA9876543210ull;
                    int k = 0;
                    for (int g = 0; g < 3; ++g)
                        for (int t = 0; t < nw; ++t)
                            if (grp[t] == g) { ps = (ps & ~(15ull << (4 * k))) | ((unsigned long long)t << (4 * k)); ++k; }
                    in.wperm_shared = ps;
                }
                in.deal_ntask = ntask;
                in.deal_cost.assign(cost.begin(), cost.end());
            }
            int* d_tabl;
            if ((rc = upload<int>(c, &in, tabl.data(), tabl.size(), &d_tabl))) { for (void* p : in.allocs) hipFree(p); return rc; }
            gd->core_hint = d_tabl;
        }
    }
    in.h_lambda0.assign(lambda0, lambda0 + L); in.h_gamma.assign(gamma, gamma + L); in.h_bidx.assign(b_idx, b_idx + L);
    in.h_lines.assign(lambda0, lambda0 + L); in.h_lines.insert(in.h_lines.end(), gamma, gamma + L);
    in.h_lines.insert(in.h_lines.end(), f, f + L); in.h_lines.insert(in.h_lines.end(), zfac, zfac + L);
    in.h_idx.assign(N_idx, N_idx + L); in.h_idx.insert(in.h_idx.end(), b_idx, b_idx + L); in.h_idx.insert(in.h_idx.end(), v_idx, v_idx + L);
    in.h_idx.push_back(voigt_method); in.h_idx.push_back(c->tune.no_multipole); in.h_idx.push_back(c->tune.multipole_min);
    if (!c->inst.empty()) {
        const Instrument& pv = c->inst.back();
        in.same_lines_as_prev = pv.h_idx == in.h_idx && pv.h_lines.size() == in.h_lines.size() &&
                                std::memcmp(pv.h_lines.data(), in.h_lines.data(), in.h_lines.size() * sizeof(double)) == 0;
    }
    analyse_generic(c, in);
    if (c->tune.lds_pad > 0) in.lds_bytes += (size_t)c->tune.lds_pad;   // occupancy experiments
    c->inst.push_back(std::move(in));
    c->meta_dirty = true;
    if (inst_index) *inst_index = (int)c->inst.size() - 1;
    return VP_OK;
}

int vp_update_spectrum(vp_ctx* c, int inst, const double* flux, const double* inv_sigma2, const double* log_inv_sigma2) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    if (inst < 0 || inst >= (int)c->inst.size()) return fail(c, VP_EINVAL, "vp_update_spectrum: instrument index out of range");
    if (!flux || !inv_sigma2 || !log_inv_sigma2) return fail(c, VP_EINVAL, "vp_update_spectrum: NULL array");
    Instrument& in = c->inst[inst];
    if (carries_sentinel(flux, in.dev.P) || carries_sentinel(inv_sigma2, in.dev.P)) c->sentinel_unsafe = true;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipMemcpy(in.d_flux, flux, (size_t)in.dev.P * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(in.d_w, inv_sigma2, (size_t)in.dev.P * sizeof(double), hipMemcpyHostToDevice));
    in.sum_logw = neumaier_sum(log_inv_sigma2, in.dev.P);
    c->meta_dirty = true;
    return VP_OK;
}

int vp_lnprob_batch_device(vp_ctx* c, int W, int D, const double* d_theta, double* d_out, void* hip_stream) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    int rc = check_batch_args(c, W, D, d_theta, d_out);
    if (rc) return rc;
    if (W == 0) return VP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = ensure_workspace(c, W))) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if ((rc = foreign_stream_fence(c, s))) return rc;
    return enqueue_lnprob(c, W, d_theta, d_out, s);
}

