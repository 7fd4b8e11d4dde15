// capi_launch.inc -- launch policy: which kernels a batch gets (tile launches, walker_kernel and its split form, far-field expansions).
// A fragment of the ONE translation unit capi.hip (included there, in order; not a header of its own).
// What a tile launch may be handed beyond its positional arguments (named at the call site; one object serves the
// GENERIC = false launch and the GENERIC = true launch behind it: each reads only its own fields)
struct TileOpts {
    const vp::InstDev* geom = nullptr;          // the launch's geometry where it is not in.dev
    int grid_z = 1;                             // (components: the line as a grid dimension)
    double* ff = nullptr;                       // GENERIC = false: far lines from the blocks' expansions
    int gen_slots = 0;                          // GENERIC = true: > 0, a grid of at most this many workgroups per tile walks the flagged walkers
    const double* theta_rebuild = nullptr;      // GENERIC = true behind walker_kernel's flux form: whole records are formed first, from D parameters a row
    int D = 0;
};
template <int OUT, bool GENERIC>
void launch_tile(const Instrument& in, const double* lc, const int* flags, double* out, int stride, int offset,
                 int W, hipStream_t s, const vp::FinalizeArgs& fin, const int* genflag, const TileOpts& o = TileOpts{}) {
    const vp::InstDev& dev = o.geom ? *o.geom : in.dev;
    const bool fast = dev.method == VP_VOIGT_FAST;
    dim3 grid(W, dev.ntiles, o.grid_z);
    dim3 block(64 * in.nwaves);
    // (almost always an empty launch: a small grid whose workgroups walk the flagged walkers -- tile_generic_kernel)
    //  where the batch before flagged none; one workgroup per walker otherwise, as a fit with damped lines needs them)
    const dim3 gg(o.gen_slots > 0 ? std::min(W, o.gen_slots) : W, dev.ntiles, o.grid_z);
    if (dev.rbot && OUT != 2) {           // NaN wavelength samples on the astropy branch: the instances that renormalise (InstDev::rbot)
        constexpr int O = OUT == 1 ? 1 : 0;
        if (GENERIC)
            hipLaunchKernelGGL((vp::tile_generic_kernel<O, false, true>), gg, block, in.lds_bytes, s, dev, lc, flags, out, stride, offset, fin, genflag, W,
                               in.lines, (const double*)nullptr, 0);
        else
            hipLaunchKernelGGL((fast ? vp::tile_kernel<1, O, false, false, true> : vp::tile_kernel<0, O, false, false, true>), grid, block, in.lds_bytes, s,
                               dev, lc, flags, out, stride, offset, fin, genflag);
        return;
    }
#ifndef VP_NO_TILE1
    if (OUT == 0 && !GENERIC && in.nwaves == 1 && o.grid_z == 1) {        // single-wave tiles: the kernel compiled for them alone
        vp::Tile1Args a{dev, lc, flags, genflag, vp::TileTail{out, stride, offset, fin}};
        a.I.ff = o.ff;
        hipLaunchKernelGGL((fast ? vp::tile_kernel1<1, false> : o.ff ? vp::tile_kernel1<0, true> : vp::tile_kernel1<0, false>), grid, block, in.lds_bytes, s, a);
        return;
    }
#endif
    if (o.ff && OUT != 2 && !GENERIC && dev.method == VP_VOIGT_WOFZ) {     // far lines from the blocks' expansions
        vp::InstDev d2 = dev;
        d2.ff = o.ff;
        hipLaunchKernelGGL((vp::tile_kernel<0, OUT == 1 ? 1 : 0, false, true>), grid, block, in.lds_bytes, s, d2, lc, flags, out, stride, offset, fin, genflag);
        return;
    }
    if (!GENERIC) {
        hipLaunchKernelGGL((fast ? vp::tile_kernel<1, OUT, false> : vp::tile_kernel<0, OUT, false>), grid, block, in.lds_bytes, s, dev, lc, flags, out,
                           stride, offset, fin, genflag);
    } else if (!fast) {
        if (OUT == 1 && o.theta_rebuild)
            hipLaunchKernelGGL((vp::tile_generic_kernel<1, true>), gg, block, in.lds_bytes, s, dev, lc, flags, out, stride, offset, fin, genflag, W,
                               in.lines, o.theta_rebuild, o.D);
        else
            hipLaunchKernelGGL((vp::tile_generic_kernel<OUT, false>), gg, block, in.lds_bytes, s, dev, lc, flags, out, stride, offset, fin, genflag, W,
                               in.lines, (const double*)nullptr, 0);
    }
}

// Can a walker inside the prior box have a line outside the fast domain (a > 0.1 or b <= 0)?
// a = gamma lambda0 / (4 pi 1e13 b) is largest at the lower bound of b.  A 10 % margin covers the
// difference between this estimate and the device arithmetic.
void analyse_generic(vp_ctx* c, Instrument& in) {
    in.needs_generic = false;
    for (size_t l = 0; l < in.h_lambda0.size(); ++l) {
        const double blo = c->h_lb.empty() ? 0.0 : c->h_lb[in.h_bidx[l]];
        if (!(blo > 0.0)) { in.needs_generic = true; return; }
        const double amax = std::fabs(in.h_gamma[l]) * in.h_lambda0[l] / (12.566370614359172 * 1e13 * blo);
        if (!(amax < 0.09) || in.h_gamma[l] < 0.0) { in.needs_generic = true; return; }
    }
}

size_t prof_mark(vp_ctx* c, hipStream_t s) {
    if (c->ev_used == c->ev_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return (size_t)-1;
        c->ev_pool.push_back(e);
    }
    const size_t i = c->ev_used++;
    (void)hipEventRecord(c->ev_pool[i], s);
    return i;
}

// Record preparation launch: one lane per record, 64 records per wave (fewer per wave measured no
// faster even at 512 walkers x 4 lines; the prep_rpw knob overrides for experiments).
// The generic-path flags of a record-preparation launch: the buffer whose turn it is, zero in its first W entries (a memset only
// where the launch before could not vouch for that), and the other buffer, which this launch clears for the next one.
struct GenFlags { int* use; int* clear; int* any; int* any_clear; int slots; };
static int genflag_acquire(vp_ctx* c, int W, hipStream_t s, GenFlags* out) {
    const int b = (int)(c->gen_seq & 1u), o = b ^ 1;
    if (!c->h_gen_any) {
        if (hipHostMalloc((void**)&c->h_gen_any, 64, hipHostMallocMapped) == hipSuccess &&
            hipHostGetDevicePointer((void**)&c->h_gen_any_dev, c->h_gen_any, 0) == hipSuccess) {
            c->h_gen_any[0] = 0;
        } else { c->h_gen_any = nullptr; c->h_gen_any_dev = nullptr; (void)hipGetLastError(); }
    }
    // No batch of this context has flagged a walker so far (ONE word, set by the launches, never cleared by them: a fit with
    // damped lines says so within its first batches and keeps one workgroup per walker from then on; batches enqueued ahead of
    // the GPU would make anything finer unreliable): this batch's generic launch will most likely be empty -- a small grid
    const bool quiet = c->h_gen_any && __atomic_load_n(&c->h_gen_any[0], __ATOMIC_RELAXED) == 0;
    int* use = c->d_genflag + (size_t)b * c->capW;
    if (c->gen_clean[b] < W) HIP_TRY(c, hipMemsetAsync(use, 0, (size_t)W * sizeof(int), s));
    c->gen_clean[b] = 0;                                   // (written by this launch)
    if (c->gen_clean[o] < W) c->gen_clean[o] = W;          // (cleared by this launch)
    ++c->gen_seq;
    *out = GenFlags{use, c->d_genflag + (size_t)o * c->capW, c->h_gen_any_dev, nullptr, quiet ? vp::GEN_SLOTS : 0};
    return VP_OK;
}
static void launch_prep(const vp_ctx* c, const Instrument& in, const double* d_theta, int W, int do_flags, double* d_out, const GenFlags& gf, hipStream_t s) {
    const long nline = (long)W * in.dev.L, ncl = (long)W * in.dev.NCm;
    const int rpw = std::max(1, std::min(64, c->tune.prep_rpw));
    vp::PrepGrid g;
    g.rpw = rpw;
    g.nb_line = (int)((nline + rpw - 1) / rpw);
    g.nb_cl = (int)((ncl + rpw - 1) / rpw);
    g.cl_wpw = 0;
    if (in.lines.M > 0 && in.lines.M <= 64 && c->tune.prep_rpw >= 64) {      // cluster records by a lane per member
        g.cl_wpw = 64 / in.lines.M;
        g.nb_cl = (W + g.cl_wpw - 1) / g.cl_wpw;
    }
    g.nb_flag = do_flags ? W : 0;
    // (direct-write gather: the pass's first launch -- the one that applies the box prior -- handshakes with the peers)
    const vp::Replicas rep = (c->gather_rep && do_flags) ? *c->gather_rep : vp::Replicas{};
    hipLaunchKernelGGL(vp::prep_lines_kernel, dim3(g.nb_line + g.nb_cl + g.nb_flag), dim3(64), 0, s, d_theta, W, c->D,
                       in.lines, c->d_lb, c->d_ub, c->d_lc, c->d_flags, do_flags, d_out, gf.use, g, rep, gf.clear, gf.any, gf.any_clear);
}

// walker_kernel: the whole batch in ONE launch (workgroup = walker, wave = tile).  Possible for a single
// instrument with single-wave tiles, at most 16 of them, whose prior box keeps every line in the fast
// domain.  A walker's workgroup holds 12 wave slots of one CU for as long as its slowest tile runs, two fit on a
// CU, so the launch time is a step function of the number of 256-workgroup layers: measured on C1 (us per pass,
// walker kernel / prep + tile + finalize launches) 64: 18.2 / 22.3, 128: 18.3 / 23.5, 256: 18.3 / 24.9,
// 320: 24.8 / 26.9, 384: 24.8 / 29.3, 512: 25.0 / 31.0, 640: 38.5 / 35.5, 768: 38.9 / 36.4, 1024: 47.3 / 43.1.
// By default it is therefore used whenever the batch fits the CUs at once (two layers on C1); larger batches keep
// the one-wave workgroups, whose slots the hardware refills one by one as tiles finish.  Instruments with multipole
// clusters (>= 3 components of a transition) run it WITHOUT cluster records, their members as ordinary lines: forming
// the records in the workgroup costs a long per-lane chain and scratch; measured on 4096 pixels, us per pass, walker
// kernel / launches: MgII doublet x 3 components 256 walkers 22.5 / 32.1, 512: 29.3 / 39.2; x 4: 28.5 / 36.5 and
// 38.6 / 49.1; FeII 4 transitions x 4: 32.2 / 38.2 and 43.7 / 51.8.
// (one or two instruments: a second one must have the first one's line tables -- the walker's records serve both)
int walker_tiles(const vp_ctx* c) {
    int n = 0;
    for (auto& in : c->inst) n += in.dev_w.ntiles;
    return n;
}
size_t walker_wave_lds(const vp_ctx* c) {
    size_t b = 0;
    for (auto& in : c->inst) b = std::max(b, in.lds_w);
    return b;
}
size_t walker_lds(int waves, size_t wave_lds) {      // tiles | tile sums, prior flag, spare | sampler form: 4 scalars, X_k, Y (64 each)
    return (size_t)waves * wave_lds + (size_t)(waves + 2 + 4 + 128) * sizeof(double);
}
size_t walker_lds_bytes(const vp_ctx* c) { return walker_lds(walker_tiles(c), walker_wave_lds(c)); }

#ifndef VP_WALKER_MAX_LINES
#define VP_WALKER_MAX_LINES 40        // above: the launches win (multipoles, far-field expansions, finer scheduling) -- 5000 pixels,
#endif                                // 256 walkers, us per pass, walker kernel / launches: 20 lines 38.7 / 49.6, 40: 67.9 / 69.9, 64: 105.8 / 99.0
bool walker_applies(const vp_ctx* c, int W) {
    if (c->tune.walker == 0 || c->inst.empty() || c->inst.size() > 4 || c->D > 64) return false;
    const Instrument& in = c->inst[0];
    for (auto& k : c->inst) {
        if (k.nanfix) return false;          // (NaN wavelength samples on the astropy branch: the tile launches' NANFIX instances)
        if (k.lds_w == 0 || k.dev.method != in.dev.method) return false;
        if (k.dev.method == VP_VOIGT_WOFZ && k.needs_generic) return false;
    }
    for (size_t k = 1; k < c->inst.size(); ++k)
        if (!c->inst[k].same_lines_as_prev || c->tune.walker_clusters) return false;
    const int nt = walker_tiles(c);
    if (nt > vp::WALKER_THREADS_MAX / 64) return false;
    if (walker_lds_bytes(c) > c->lds_limit) return false;
    if (c->tune.walker == 1) return true;
    if (in.dev.L > VP_WALKER_MAX_LINES || (in.dev.NCm > 0 && c->tune.walker_clusters)) return false;
    // LSFs of more than 33 taps: the launches use 2- or 4-wave tile workgroups, the walker kernel single-wave tiles with
    // more halo -- measured on 2100 pixels, us per pass, launches / walker kernel: 45 taps 64 walkers 17.8 / 18.1,
    // 256: 20.5 / 18.2, 512: 26.9 / 22.0; 101 taps 19.4 / 22.1, 23.9 / 22.2, 35.0 / 32.1
    for (auto& k : c->inst)
        if (k.nwaves != 1 && W < 192) return false;
    // a CU holds per_cu walker workgroups at once (24 wave slots / waves per walker, LDS permitting); the batch lies
    // on the 256 CUs in layers of 256 workgroups and the launch takes as long as the fullest CU's layers
    const int per_cu = std::max(1, std::min(24 / std::max(1, nt), (int)(c->lds_limit / walker_lds_bytes(c))));
    // (short spectra: more workgroups fit on a CU and more layers stay ahead of the launches -- C1 cut to 1400 pixels, 4
    // tiles, 1024 walkers 22.0 vs 29.2 us; 2100 pixels, 6 tiles: 768 walkers 22.7 vs 30.1, 1024: 39.3 vs 33.5; 2800 pixels,
    // 8 tiles: 768 walkers 26.4 vs 33.6, 1024: 38.0 vs 37.6)
    const int layers = (W + 255) / 256;
    // (two workgroups per CU -- C1's 12 tiles --: a batch that fills a second round of 512 workgroups is still better off than
    //  through the launches -- C1, us per pass, walker kernel / launches: 768 walkers 35.5 / 36.1, 896: 41.7 / 42.5, 1024: 41.9 /
    //  44.75; 576: 35.2 / 29.9, 640: 35.3 / 32.1, 1280: 55.5 / 51.6)
    if (per_cu == 2 && layers == 4) return true;
    return layers <= per_cu && (layers <= 3 || layers <= per_cu - 2);
}

int ctx_num_cus(vp_ctx* c) {
    if (c->num_cus == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess) c->num_cus = n;
    }
    return c->num_cus;
}
// walker_kernel's split form (WalkerArgs::split): how many workgroups a walker of a W-row batch gets, 0 = the ordinary form.
// Where a batch leaves CUs without a workgroup the launch is as long as its heaviest wave's chain (profiles/r05_C1_budget.txt:
// entry 5.0 + phase-A skeleton 3.0 + line cores 3.3 us of 15.5 at 256 walkers); one-pass tiles shorten the chain behind the entry,
// and several workgroups per walker put them on the idle CUs.
int walker_split_for(vp_ctx* c, int W) {
    if (c->tune.walker_split == 0 || c->inst.size() != 1 || c->tune.walker_clusters || c->gather_rep) return 0;
    const Instrument& in = c->inst[0];
    if (in.lds_s == 0 || !in.split_hint) return 0;
    const int nt = in.dev_s.ntiles, ncu = ctx_num_cus(c);
    int G = c->tune.walker_split;
    if (G < 0) {
        // Measured on C1 (us per pass, ordinary form / 2 / 4 / 8 groups; profiles/r05_experiments/split_sweep.txt): 16 walkers 15.25 /
        // 15.90 / 15.47 / 13.99, 32: 15.29 / 15.88 / 15.51 / 14.05, 50: 15.35 / 15.93 / 15.55 / 15.89, 64: 15.37 / 16.00 / 15.71 / 16.21,
        // 128: 15.42 / 16.06 / 18.52 / 19.77, 256: 15.42 / 27.99 (two 13-wave workgroups do not fit a CU's wave slots together) --
        // the form pays only where every group gets a CU's SIMDs to itself (one wave per SIMD): the launch is a 5.5 us entry plus
        // the heaviest wave's own latency chain (60 % of a lone wave's cycles are s_waitcnt), which one-pass tiles shorten by a
        // third, not by half.  So: eight groups where W x 8 workgroups still leave every CU at most one, nothing above.
        if (ncu <= 0 || (long)W * 8 > ncu) return 0;
        G = 8;
    }
    G = std::min(G, nt);
    if (G < 2 || (long)W * G > 1024) return 0;
    const int nwpg = (nt + G - 1) / G;
    if (nwpg > vp::WALKER_THREADS_MAX / 64) return 0;
    if (walker_lds(nwpg, in.lds_s) > c->lds_limit) return 0;
    return G;
}
struct SplitShape { int G, waves; size_t lds; };
SplitShape split_shape(const vp_ctx* c, int G) {
    const Instrument& in = c->inst[0];
    const int nwpg = (in.dev_s.ntiles + G - 1) / G;
    return SplitShape{G, nwpg, walker_lds(nwpg, in.lds_s)};
}

// (clusters: without their multipole records the members are ordinary lines -- a few more wing evaluations per pass
// against a cluster preparation chain inside every workgroup)
// a.split > 0: the split form -- W x split workgroups on the one-pass geometry; a.split_row0: first row of the tile-sum / ticket
// workspace this launch may use (the record rows come with a.lc)
template <bool SAMPLER, bool ARMED = false>
void launch_walker_any(vp_ctx* c, int W, const vp::WalkerArgs& a, const vp::StretchArgs& st, hipStream_t s) {
    const Instrument& in = c->inst[0];
    const bool fast = in.dev.method == VP_VOIGT_FAST;
    if (a.split > 0) {
        const SplitShape sh = split_shape(c, a.split);
        vp::InstDev d0 = in.dev_s;
        vp::LinesDev t0 = in.lines;
        d0.NCm = 0; t0.NCm = 0;
        d0.core_hint = in.split_hint;
        d0.ff = nullptr;
        hipLaunchKernelGGL((fast ? vp::walker_kernel<1, false, SAMPLER, ARMED, 0, true> : vp::walker_kernel<0, false, SAMPLER, ARMED, 0, true>),
                           dim3(W * a.split), dim3(64 * sh.waves), sh.lds, s, d0, t0, a, st);
        return;
    }
    const dim3 grid(W), block(64 * walker_tiles(c));
    const size_t lds = walker_lds_bytes(c);
    vp::InstDev d0 = in.dev_w;
    vp::LinesDev t0 = in.lines;
    const bool keep_clusters = in.dev.NCm > 0 && c->tune.walker_clusters && !SAMPLER && c->inst.size() == 1;
    if (!keep_clusters) { d0.NCm = 0; t0.NCm = 0; }
    if (c->inst.size() > 1) {
        vp::InstDev dk[4] = {d0, d0, d0, d0};
        vp::WalkerMore tb{};
        int tsum = d0.ntiles;
        for (size_t k = 1; k < c->inst.size(); ++k) {
            dk[k] = c->inst[k].dev_w;
            dk[k].NCm = 0;
            tb.t[k - 1] = tsum;
            tb.slw[k - 1] = c->inst[k].sum_logw;
            tsum += dk[k].ntiles;
        }
        for (size_t k = c->inst.size(); k < 4; ++k) tb.t[k - 1] = tsum;        // (no tiles)
        if (c->inst.size() == 2)
            hipLaunchKernelGGL((fast ? vp::walker_kernel2<1, SAMPLER, ARMED> : vp::walker_kernel2<0, SAMPLER, ARMED>), grid, block, lds, s, dk[0], dk[1], tb, t0, a, st);
        else
            hipLaunchKernelGGL((fast ? vp::walker_kernel4<1, SAMPLER, ARMED> : vp::walker_kernel4<0, SAMPLER, ARMED>), grid, block, lds, s, dk[0], dk[1], dk[2], dk[3],
                               tb, t0, a, st);
        return;
    }
    hipLaunchKernelGGL((fast ? vp::walker_kernel<1, false, SAMPLER, ARMED> : keep_clusters ? vp::walker_kernel<0, true, false, ARMED>
                                                                                            : vp::walker_kernel<0, false, SAMPLER, ARMED>),
                       grid, block, lds, s, d0, t0, a, st);
}

// which deal of tiles to waves a walker launch of W workgroups gets (Tuning::walker_perm).  At most one workgroup per CU: the cost deal
// (Instrument::wperm).  More -- 257 ... 512 walkers and the second round up to 1024 on C1's 12 tiles --: the grid-order deal with the
// line-core tiles behind the entry waves (Instrument::wperm_shared; the identity before: C1 at 512 walkers 21.20 -> 20.80 us per pass,
// profiles/simd_deal_notes.md).  shared_ok: the plain and the sampler form of the one-instrument launch; the pre-armed and the flux
// form keep the identity there.
unsigned long long walker_deal_for(vp_ctx* c, int W, bool shared_ok) {
    const unsigned long long ident = 0xFEDCBA9876543210ull;
    const int mode = c->tune.walker_perm;
    if (c->inst.size() != 1 || mode == 0) return ident;
    if (c->tune.walker_perm_hex != 0) return (unsigned long long)c->tune.walker_perm_hex;     // (experiments: an explicit deal)
    const Instrument& in = c->inst[0];
    if (mode == 1) return in.wperm;
    if (mode == 2 && shared_ok) return in.wperm_shared;
    if (ctx_num_cus(c) > 0 && W <= ctx_num_cus(c)) return in.wperm;
    return shared_ok ? in.wperm_shared : ident;
}
// raised issue priority for the waves with line cores: where workgroups share a CU (WalkerArgs::prio)
int walker_prio_for(vp_ctx* c, int W) {
    if (c->tune.walker_prio >= 0) return c->tune.walker_prio ? 1 : 0;
    return (ctx_num_cus(c) > 0 && W <= ctx_num_cus(c)) ? 0 : 1;
}

// The WalkerArgs of every form of the launch: W walkers that read `theta` and write `out` (both nullptr in the sampler form, whose
// rows come with StretchArgs); split > 0: the split form, W x split workgroups whose rows of the tile-sum / ticket workspace begin at
// row0 -- every workgroup of a walker has its own record rows, so a second launch in flight starts behind row0 x split of them;
// shared_cus: another launch sits on the CUs at the same time (overlapped half-steps)
vp::WalkerArgs walker_args(vp_ctx* c, int W, const double* theta, double* out, double sum_logw, int split = 0, int row0 = 0,
                           bool shared_cus = false, bool shared_ok = false) {
    const Instrument& in = c->inst[0];
    const size_t nrec = (size_t)(in.dev.L + in.dev.NCm) * vp::LC_STRIDE;
    const int per = std::max(1, split);
    vp::WalkerArgs a{theta, c->d_lb, c->d_ub, c->d_lc + (size_t)row0 * per * nrec, out, sum_logw, c->D,
                     (int)((split > 0 ? in.lds_s : walker_wave_lds(c)) / sizeof(double)),
                     (shared_cus && c->tune.walker_prio < 0) ? 1 : walker_prio_for(c, W * per),     // (overlapped half-steps share the CUs)
                     split > 0 ? 0xFEDCBA9876543210ull : walker_deal_for(c, W, shared_ok)};
    if (split > 0) { a.split = split; a.split_row0 = row0; a.split_part = c->d_partial; a.split_ticket = c->d_ticket; }
    return a;
}

// What a batch gets, decided once (plan_lnprob) and then launched as decided (enqueue_plan); record_launch keeps what the
// introspection calls report.
struct LaunchPlan {
    int kind = 0;            // vp_last_launch_kind: 0 prep + tile (+ finalize) launches, 1 walker_kernel, 2 the launches with far-field expansions,
                             // 3 all instruments' tiles in one launch (tile_kernel_multi); < 0: not an lnprob batch (model flux)
    int split = 0;           // walker_kernel: workgroups per walker of its split form (0: the ordinary form)
    int Wp = 0;              // rows the structure is chosen for
    int sel = 0;             // geometry of the tile launches: 0 full-size tiles (Instrument::dev), 1 one-pass tiles (dev_s), 2 single-wave tiles (dev_w)
    int fmode = 0;           // final reduction: 0 a launch of its own, 1 by ticket in the tile kernel
    int ff_first = -1;       // first instrument that takes far-field expansions (ff_wanted answers for the others) ...
    int ff_first_blk = 0;    // ... and the blocks per row that the instruments before it have in the workspace
};
const vp::InstDev& geom_of(const Instrument& x, int sel) { return sel == 2 ? x.dev_w : sel ? x.dev_s : x.dev; }

void launch_walker(vp_ctx* c, const LaunchPlan& p, int W, const double* d_theta, double* d_out, hipStream_t s, bool armed = false) {
    vp::WalkerArgs a = walker_args(c, W, d_theta, d_out, c->inst[0].sum_logw, p.split, 0, false, !armed);
    if (armed) {
        a.arm_slots = c->arm.slots;
        a.arm_slot_doubles = c->arm.slot_doubles;
        a.arm_host = c->arm.h_dev;
        a.arm_seq = c->arm.seq;
        // (100 MHz clock.  The caller's own rhythm: one and a half times its recent gap between calls + 10 us, at least 20 us, at most prearm_us --
        //  itself at most 100 ms, far below the other waves' own bound of ~1 s of polling, SYNC_SPIN_LIMIT.  "prearm" = 1 -- tests,
        //  experiments -- waits the whole prearm_us.)
        const int cap = std::min(std::max(1, c->tune.prearm_us), 100000);
        c->arm.budget_us = c->tune.prearm > 0 ? cap : std::min(cap, std::max(20, (int)(1.5 * c->arm.gap_ema_us) + 10));
        a.arm_ticks = 100 * c->arm.budget_us;
    }
    vp::StretchArgs st{};
    if (c->gather_rep) st.rep = *c->gather_rep;      // (the plain form's only use of the sampler arguments: where the results go)
    if (armed) launch_walker_any<false, true>(c, W, a, st, s);
    else launch_walker_any<false>(c, W, a, st, s);
}

// One stretch-move half-step of the active half (nS walkers) as ONE launch: proposal, lnprob and accept/reject inside
// each walker's workgroup (walker_kernel<.., SAMPLER = true>).
// (lc_row0: first row of the record workspace this launch may use -- two half-steps in flight at once, vp_stretch_run's
//  overlapped form, must not share rows)
void launch_walker_stretch(vp_ctx* c, int nS, const vp::StretchArgs& st, hipStream_t s, int lc_row0 = 0, int split = 0) {
    launch_walker_any<true>(c, nS, walker_args(c, nS, nullptr, nullptr, c->inst[0].sum_logw, split, lc_row0, st.ovl != 0, true), st, s);
}
// whole half-step in one launch (proposal, lnprob, accept inside each walker's workgroup) where the walker kernel
// applies to a half-ensemble batch and the instrument has no cluster records
// (vp_multi_stretch_run asks for the WHOLE half too: every context's block gets the form, hence the bits, one context gives the half)
// returns -1 where it is not, else a walker of the half-step as several workgroups (WalkerArgs::split; 0: the ordinary form)
int stretch_split(vp_ctx* c, int half) {
    const bool one_launch = !c->tune.no_fused_accept && c->tune.walker != 0 && walker_applies(c, half) &&
                            (c->inst[0].dev.NCm == 0 || !c->tune.walker_clusters);
    return one_launch ? walker_split_for(c, half) : -1;
}

// ---- several instruments with one set of records, small batch: all their tiles in ONE launch (tile_kernel_multi)
bool tile_multi_applies(const vp_ctx* c, int Wp) {
    const size_t ni = c->inst.size();
    bool multi = !c->profiling && ni >= 2 && ni <= 4 && c->tune.tile_multi != 0 && !c->tune.no_shared_prep;
    long waves = 0;
    for (size_t k = 0; multi && k < ni; ++k) {
        const Instrument& in = c->inst[k];
        if (k > 0 && !in.same_lines_as_prev) multi = false;
        if (in.lds_w == 0 || in.dev.method != c->inst[0].dev.method || in.nanfix) multi = false;
        if (in.needs_generic && in.dev.method == VP_VOIGT_WOFZ) multi = false;
        waves += (long)Wp * in.dev_w.ntiles;
    }
    // (measured on C3, two instruments of 8192 pixels = 52 single-wave tiles per walker, us per pass, launches / one launch:
    //  64 walkers 67.5 / 47.6, 256: 89.2 / 92.5, 512: 143.1 / 143.9, 1024: 229 / 251, 2048: 401 / 468 -- the long LSF's tiles carry
    //  more halo as single waves, which only a batch that leaves the GPU mostly idle does not feel)
    if (multi && c->tune.tile_multi < 0 && waves > 6144) multi = false;
    return multi;
}

// Far-field expansions: does the extra launch pay for an instrument?
// (the extra launch costs ~20 us; what it saves grows with walkers x blocks x lines -- measured on C2, us per pass
// without / with: 128 walkers 54.8 / 60.5, 256 (0.42e6): 72.7 / 71.5, 512: 111.8 / 98.3, 1024: 188.8 / 153.1,
// 2048: 349.0 / 260.5.  Below that the lines are walked directly unless "farfield" = 1 asks for the expansions.
// What the expansions save is one evaluation per pass for every ITEM they cover (a multipole cluster or a line
// outside clusters: C2 has 9, a 40-line FeII fit of 8 clusters 8, one of 20 lines 4), ff_cover of them (estimated
// when the instrument is added); the crossover sits near 2e5 covered (walker, block, item) triples: C2 at 256
// walkers (0.195e6) 72.7 / 71.5 us, the 40-line FeII fit at 1024 walkers (0.17e6) 164.9 / 161.1, the 20-line one
// at 1024 (0.09e6) 90.4 / 93.2.
// (round 3, after the launch itself got cheaper -- records staged in LDS, faster record preparation in front of it --: on
//  from 1.5e5 covered triples: C2 at 256 walkers (1.95e5) 57.2 / 54.9, C4 at 64 (0.9e5) 119.5 / 130.8.)
// (instruments that share their records come in pairs whose expansions are ONE launch: the pair's triples count together
//  -- C3, us per pass without / with: 128 walkers 66.4 / 70.3, 256: 68.5 / 67.0, 512: 103.8 / 94.4)
double ff_score(const Instrument& x, const vp::InstDev& gx, int Wp) {
    return x.ff_on ? x.ff_cover * (double)Wp * gx.ntiles * gx.ff_nblk * x.ff_items : 0.0;
}
bool ff_pays(const vp::InstDev& gx, double score) {
    // (instruments whose cluster members enter the expansions line by line pay more for the launch: C4 at 64 walkers
    //  -- 1.8e5 -- 119.5 / 130.3 us, at 512 walkers 636 / 529)
    return score >= (gx.ff_members ? 3.0e5 : 1.5e5);
}
bool ff_wanted(const vp_ctx* c, const LaunchPlan& p, size_t i) {
    const Instrument& x = c->inst[i];
    if (!x.ff_on || !c->d_ff || c->tune.farfield == 0) return false;
    if (c->tune.farfield > 0) return true;
    const vp::InstDev& gx = geom_of(x, p.sel);
    double score = ff_score(x, gx, p.Wp);
    if (!c->tune.no_shared_prep && !c->profiling) {
        size_t r0 = i;
        while (r0 > 0 && c->inst[r0].same_lines_as_prev) --r0;
        const size_t partner = r0 + ((i - r0) ^ 1);
        const bool in_run = partner < c->inst.size() && (partner < i ? true : c->inst[partner].same_lines_as_prev) &&
                            (partner > i || c->inst[i].same_lines_as_prev);
        if (in_run && geom_of(c->inst[partner], p.sel).ff_members == gx.ff_members)
            score += ff_score(c->inst[partner], geom_of(c->inst[partner], p.sel), p.Wp);
    }
    return ff_pays(gx, score);
}
// the next instrument's too, in the same launch, when it has these line tables (the same records)
bool ff_paired(const vp_ctx* c, const LaunchPlan& p, size_t k) {
    const Instrument* nx = (k + 1 < c->inst.size() && !c->profiling) ? &c->inst[k + 1] : nullptr;
    return nx && nx->same_lines_as_prev && !c->tune.no_shared_prep && ff_wanted(c, p, k + 1) &&
           geom_of(*nx, p.sel).ff_members == geom_of(c->inst[k], p.sel).ff_members;
}
// the tile offsets and weights the finalize launch takes by value (n_inst = 0: more instruments than it holds -- the launch reads them from memory)
vp::FinalizeByValue finalize_by_value(const vp_ctx* c, const LaunchPlan& p) {
    vp::FinalizeByValue bv{};
    const size_t ni = c->inst.size();
    if (ni > (size_t)vp::FIN_MAX_INST) return bv;
    bv.n_inst = (int)ni;
    int off = 0;
    for (size_t k = 0; k < ni; ++k) {
        bv.tile_off[k] = off;
        off += geom_of(c->inst[k], p.sel).ntiles;
        bv.sum_logw[k] = c->inst[k].sum_logw;
    }
    bv.tile_off[ni] = off;
    return bv;
}
// plan kind 3: one record-preparation launch, all instruments' tiles in one launch, the final reduction
void enqueue_tile_multi(vp_ctx* c, const LaunchPlan& p, int W, const double* d_theta, double* d_out, const vp::FinalizeArgs& fin, hipStream_t s) {
    const size_t ni = c->inst.size();
    const Instrument& in0 = c->inst[0];
    launch_prep(c, in0, d_theta, W, 1, d_out, GenFlags{}, s);
    vp::InstDev dk[4] = {in0.dev_w, in0.dev_w, in0.dev_w, in0.dev_w};
    vp::TileMulti tb{};
    int tsum = 0;
    for (size_t k = 0; k < ni; ++k) {
        dk[k] = c->inst[k].dev_w;
        tb.off[k] = tsum;
        if (k > 0) tb.t[k - 1] = tsum;
        tsum += dk[k].ntiles;
    }
    for (size_t k = ni; k < 4; ++k) { tb.t[k - 1] = tsum; tb.off[k] = tsum; }
    const int nt = fin.total_tiles;
    hipLaunchKernelGGL((in0.dev.method == VP_VOIGT_FAST ? vp::tile_kernel_multi<1> : vp::tile_kernel_multi<0>), dim3(W, nt), dim3(64), walker_wave_lds(c), s,
                       dk[0], dk[1], dk[2], dk[3], tb, (int)ni, c->d_lc, c->d_flags, c->d_partial, nt, fin);
    if (!p.fmode)        // (two to four instruments: always by value)
        hipLaunchKernelGGL((vp::finalize_kernel<true>), dim3((W + 63) / 64), dim3(64), 0, s, c->d_partial, nt, W, c->d_flags, fin, finalize_by_value(c, p),
                           c->gather_rep ? *c->gather_rep : vp::Replicas{});
}
// the blocks' far-field expansions of instrument k from the records just made, into ff; paired: and behind them, in the same launch,
// those of instrument k + 1
void launch_farfield(const vp_ctx* c, const LaunchPlan& p, size_t k, double* ff, bool paired, int W, hipStream_t s) {
    const Instrument& in = c->inst[k];
    vp::InstDev g2 = geom_of(in, p.sel), g3 = geom_of(c->inst[paired ? k + 1 : k], p.sel);
    const int nbk = g2.ntiles * g2.ff_nblk, nbx0 = (nbk + 63) / 64, nbx1 = (g3.ntiles * g3.ff_nblk + 63) / 64;
    g2.ff = ff;
    g3.ff = ff + (size_t)W * nbk * vp::FF_STRIDE;
    const size_t ffl = vp::farfield_lds_bytes(in.lines.L, in.lines.NCm);
    const dim3 block(64 * vp::FF_WAVES);
    if (paired)
        hipLaunchKernelGGL((g2.ff_members ? vp::farfield_kernel2<9, true> : vp::farfield_kernel2<6, false>), dim3(nbx0 + nbx1, W), block, ffl, s, g2, g3, nbx0,
                           in.lines, c->d_lc, W);
    else
        hipLaunchKernelGGL((g2.ff_members ? vp::farfield_kernel<9, true> : vp::farfield_kernel<6, false>), dim3(nbx0, W), block, ffl, s, g2, in.lines, c->d_lc, W);
}
// Which launches a batch gets, for Wp rows (a block of a larger batch that other contexts share is planned for the whole batch's rows:
// same structure, hence the same bits, as the whole batch on one context).  Reads the context, writes nothing.
LaunchPlan plan_lnprob(vp_ctx* c, int Wp) {
    LaunchPlan p;
    p.Wp = Wp;
    if (walker_applies(c, Wp)) {
        p.kind = 1;
        p.split = walker_split_for(c, Wp);
        return p;
    }
    // Geometry: a batch whose full-size tiles would leave most wave slots empty is cut into one-pass
    // tiles instead (twice the workgroups, half the per-wave latency): measured better up to 384
    // walkers x 12 tiles (30.2 vs 31.1 us), equal at 448, worse at 512 (256 CUs x 4 SIMDs x 6 waves =
    // 6144 slots).
    p.sel = ((long)Wp * c->total_tiles_g[0] <= 4800) ? 1 : 0;
    if (c->tune.geom >= 0) p.sel = c->tune.geom ? 1 : 0;
    // Final reduction (bit-identical either way, see tile_kernel): fused into the tile kernel -- the
    // last-arriving tile of a walker, by ticket -- while the batch leaves wave slots empty; a small launch of
    // its own (one lane per walker) once the batch fills them, where the ticket's L2 round trips at the end of
    // every tile wave cost more than a launch.  Measured on C1 (us per pass, own launch / ticket): 256
    // walkers 26.5 / 26.7, 512: 32.3 / 33.0-33.9, 2048: 88.9 / 92.5, 8192: 314 / 329.
    p.fmode = ((long)Wp * c->total_tiles_g[0] < 6144) ? 1 : 0;
    if (tile_multi_applies(c, Wp)) {
        p.kind = 3;
        p.sel = 2;
        // (final reduction by its own launch: with these many single-wave tiles per walker the ticket's round trips at the
        //  end of every wave cost more -- C3 at 64 walkers 56.9 us by ticket, 47.6 by launch; scripts/structure_check.py)
        p.fmode = 0;
    }
    if (c->tune.finalize >= 0) p.fmode = c->tune.finalize ? 1 : 0;      // 0: own launch, 1: ticket
    if (c->gather_rep) p.fmode = 0;                  // (the finalize launch is what writes into the ranks' gathered vectors)
    // every instrument's expansions have their own stretch of the workspace (W x its blocks), in instrument order
    for (size_t k = 0, blk = 0; p.kind == 0 && k < c->inst.size(); ++k) {
        const vp::InstDev& gk = geom_of(c->inst[k], p.sel);
        if (ff_wanted(c, p, k)) { p.kind = 2; p.ff_first = (int)k; p.ff_first_blk = (int)blk; }
        if (c->inst[k].ff_on) blk += (size_t)gk.ntiles * gk.ff_nblk;
    }
    return p;
}
// what vp_last_launch_kind, vp_last_walker_split and vp_last_farfield_info report of a batch of W rows launched by plan p
void record_launch(vp_ctx* c, const LaunchPlan& p, int W) {
    if (p.kind >= 0) { c->last_kind = p.kind; c->last_split = p.split; }
    c->last_ff = vp_ctx::LastFF{};
    if (p.ff_first < 0) return;
    const vp::InstDev& g = geom_of(c->inst[p.ff_first], p.sel);
    c->last_ff = vp_ctx::LastFF{c->d_ff + (size_t)W * p.ff_first_blk * vp::FF_STRIDE, W, g.ntiles * g.ff_nblk, g.ff_members, p.ff_first};
}
// enqueue the launches of plan p for W rows of device-resident theta / out
int enqueue_plan(vp_ctx* c, const LaunchPlan& p, int W, const double* d_theta, double* d_out, hipStream_t s) {
    const bool prof = c->profiling;
    size_t m0 = prof ? prof_mark(c, s) : 0;
    if (p.kind == 1) {
        launch_walker(c, p, W, d_theta, d_out, s);
        if (prof) {
            size_t m1 = prof_mark(c, s);
            c->spans.push_back({m0, m1, 1});
        }
        HIP_TRY(c, hipGetLastError());
        return VP_OK;
    }
    const size_t ni = c->inst.size();
    const int ntot = p.sel == 2 ? c->total_tiles_w : c->total_tiles_g[p.sel];
    const vp::FinalizeArgs fin{c->d_ticket, c->d_tile_off + p.sel * (ni + 1), c->d_sum_logw, d_out, (int)ni, ntot, p.fmode};
    if (p.kind == 3) {
        enqueue_tile_multi(c, p, W, d_theta, d_out, fin, s);
        HIP_TRY(c, hipGetLastError());
        return VP_OK;
    }
    int tile_off = 0;
    size_t ff_blk = 0;                               // blocks per row the expansions of the instruments so far have in the workspace
    bool ff_made = false;                            // this instrument's expansions came with the previous one's launch
    GenFlags gf{c->d_genflag, nullptr, nullptr, nullptr, 0};     // (the flags of the records in the workspace: shared by instruments that share those)
    int rc_gf = VP_OK;
    for (size_t k = 0; k < ni; ++k) {
        const Instrument& in = c->inst[k];
        const bool gen = in.needs_generic && in.dev.method == VP_VOIGT_WOFZ;
        if (!(k > 0 && in.same_lines_as_prev && !c->tune.no_shared_prep)) {       // (same line tables as the previous instrument: its records and
                                                       // generic-path flags are still in the workspace)
            if (gen && (rc_gf = genflag_acquire(c, W, s, &gf))) return rc_gf;
            launch_prep(c, in, d_theta, W, k == 0 ? 1 : 0, d_out, gen ? gf : GenFlags{}, s);
        }
        const vp::InstDev& geom = geom_of(in, p.sel);
        TileOpts o;
        o.geom = &geom;
        o.ff = ff_wanted(c, p, k) ? c->d_ff + (size_t)W * ff_blk * vp::FF_STRIDE : nullptr;
        o.gen_slots = gf.slots;
        if (in.ff_on) ff_blk += (size_t)geom.ntiles * geom.ff_nblk;
        const bool ff_launch = o.ff && !ff_made;
        ff_made = ff_launch && ff_paired(c, p, k);       // (consumed by the next instrument's pass of this loop)
        if (ff_launch) launch_farfield(c, p, k, o.ff, ff_made, W, s);
        size_t m1 = prof ? prof_mark(c, s) : 0;
        launch_tile<0, false>(in, c->d_lc, c->d_flags, c->d_partial, ntot, tile_off, W, s, fin, gen ? gf.use : (const int*)nullptr, o);
        if (gen) launch_tile<0, true>(in, c->d_lc, c->d_flags, c->d_partial, ntot, tile_off, W, s, fin, gf.use, o);
        if (prof) {
            size_t m2 = prof_mark(c, s);
            c->spans.push_back({m0, m1, 0});
            c->spans.push_back({m1, m2, 1});
            m0 = m2;
        }
        tile_off += geom.ntiles;
    }
    if (!p.fmode) {
        const vp::FinalizeByValue bv = finalize_by_value(c, p);
        hipLaunchKernelGGL((bv.n_inst ? vp::finalize_kernel<true> : vp::finalize_kernel<false>), dim3((W + 63) / 64), dim3(64), 0, s, c->d_partial, ntot, W,
                           c->d_flags, fin, bv, c->gather_rep ? *c->gather_rep : vp::Replicas{});
        if (prof) {
            size_t m3 = prof_mark(c, s);
            c->spans.push_back({m0, m3, 2});
        }
    }
    HIP_TRY(c, hipGetLastError());
    return VP_OK;
}

// enqueue the whole lnprob pipeline for device-resident theta / out: per instrument a prep launch
// (line records; the first one also applies the box prior and writes -inf rows) and a tile launch;
// the last-arriving tile workgroup of each walker performs the final reduction.
// Wp > 0: the rows the launch structure is chosen for, where they are not the batch's own (LaunchPlan::Wp)
int enqueue_lnprob(vp_ctx* c, int W, const double* d_theta, double* d_out, hipStream_t s, int Wp = 0) {
    const LaunchPlan p = plan_lnprob(c, Wp > 0 ? Wp : W);
    record_launch(c, p, W);
    return enqueue_plan(c, p, W, d_theta, d_out, s);
}
