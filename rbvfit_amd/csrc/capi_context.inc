// capi_context.inc -- context, tuning knobs, instruments, per-batch workspace.
// A fragment of the ONE translation unit capi.hip (included there, in order; not a header of its own).
namespace {

thread_local std::string g_create_error;
#ifdef VP_STAMPS
// diagnostic build: wall-clock stamps of the last vp_lnprob_batch call (ns since its entry): 0 theta staged, 1 launches enqueued,
// 2 first output row seen, 3 all rows seen / completion, 4 copied out
double g_host_stamps[8];
std::chrono::steady_clock::time_point g_host_t0;
#define VP_HSTAMP(k) g_host_stamps[k] = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - g_host_t0).count()
#else
#define VP_HSTAMP(k) do { } while (0)
#endif

// Tuning / experiment knobs.  Defaults come from RBVFIT_AMD_* environment variables read ONCE, when the
// context is created (never on the per-call path); vp_set_option changes them per context.
struct Tuning {
    int prep_rpw = 64;          // records per wave of prep_lines_kernel
    int geom = -1;              // tile geometry: -1 by batch size, 0 two-pass tiles, 1 one-pass tiles
    int finalize = -1;          // final reduction: -1 by batch size, 0 own launch, 1 ticket in the tile kernel
    int walker = -1;            // walker_kernel (one launch per batch): -1 by batch size, 0 never, 1 whenever possible
    long zerocopy_max = 1l << 20;    // bytes of theta up to which the host entry reads pinned host memory directly
    int no_zerocopy = 0;
    int no_multipole = 0;       // (read when an instrument is added)
    int multipole_min = 3;      // smallest cluster (components of one transition) that gets a multipole record
                                // (2 measured slower on C1: 35.6 vs 32.2 us per 512-walker pass -- the attempt costs an
                                // un-prefetched record fetch per cluster and pass, and the prep launch grows)
    int span = 0;               // evaluated pixels per tile, 0 = default (read when an instrument is added)
    int waves = 0;              // waves per tile workgroup, 0 = default (read when an instrument is added)
    long lds_pad = 0;           // extra LDS bytes per tile workgroup: occupancy experiments
    int no_fused_accept = 0;    // device sampler: separate accept / propose launches
    int farfield = -1;          // far-field expansions in the tile launches: -1 for instruments with >= 8 lines and batches
                                // with enough covered (walker, block, item) triples (enqueue_lnprob), 0 never, 1 whenever possible (the instrument's
                                // block tables are made when it is added: 0 at that time rules them out for good)
    int no_shared_prep = 0;     // instruments with the previous one's line tables prepare their records again anyway
    int walker_clusters = 0;    // walker_kernel on instruments with multipole clusters: 0 = walk the member lines one by one
                                // (no cluster records: the plain instance), 1 = cluster records formed in the workgroup
                                // (that instance spills to scratch)
    int multi_sync = 0;         // vp_multi_stretch_run: how the contexts' half-steps are ordered (read from context 0): 0 events between
                                // their streams (default), 1 flags polled inside the kernels -- no host call and no cross-queue wait per
                                // half-step; tested with the contexts on ONE device, where it measured no faster than events because the
                                // contexts' kernels share the CUs (C1, 2 contexts: 49.9 vs 39.5 us per half-step; C3 at 2048 walkers:
                                // 257 vs 272); across devices it uses system-scope fences and has never run
    int host_spin = 2;          // how the host-buffer entries learn that their batch is done: 0 hipStreamSynchronize; 1 spin on a host-mapped
                                // completion word the stream writes behind the batch (512-walker C1 call 42.7 -> ~39.5 us); 2 zero-copy batches:
                                // spin on the OUTPUT ROWS themselves -- they are pre-set to a NaN pattern no arithmetic produces and every
                                // row is written exactly once, by the launch that finishes it: no completion packet behind the kernel and no
                                // hipStreamWriteValue32 call in front of it (falls back to 1 when an input carries that pattern)
    int no_ff_members = 0;      // (read when an instrument is added) never take cluster members into the far-field expansions one by one
    int tile_multi = -1;        // tiles of several instruments in one launch (tile_kernel_multi): -1 by batch size, 0 never, 1 whenever possible
    int gather_plain = 0;       // vp_gather_create: ordinary device memory for the gathered vector and flags instead of fine-grained
    int tile_lpt = 1;           // (read when an instrument is added) tile launches hand out the tiles with the most line cores
                                // first (0: in grid order)
    int slice_rows = 2;         // device slice sampler: rows of a round's lnprob batch per walker of the half-ensemble (2 ... 8)
    int flux_farfield = -1;     // vp_model_flux_batch[_device]: far lines from the blocks' expansions as in the lnprob launches: -1 by batch
                                // size (the lnprob rule), 0 never, 1 whenever the instrument has the tables
    int walker_prio = -1;       // walker_kernel: raised issue priority for the waves with line cores: -1 where workgroups share a CU, 0 never, 1 always
    long walker_perm_hex = 0;   // (experiments) an explicit WalkerArgs::wperm
    int walker_perm = -1;       // walker_kernel deals its tiles to the waves by estimated cost (WalkerArgs::wperm): -1 by batch size (at most
                                // one workgroup per CU: the cost deal; more: the grid-order deal with the line-core tiles behind the entry
                                // waves, walker_deal_for), 0 never (wave k takes tile k), 1 always the cost deal, 2 always the grid-order deal
    int stretch_overlap = -1;   // vp_stretch_run, half-steps as one launch each: -1 consecutive half-steps on two streams, ordered walker by
                                // walker through version words (StretchArgs::ovl), where two half-ensembles fit the CUs at once; 0 never
                                // (every half-step behind the one before, one stream); 1 whenever the half-steps are one launch each
    int prearm = -1;            // vp_lnprob_batch, batches that are ONE walker_kernel launch: the launch for the NEXT call is put on the GPU
                                // while this call's runs, waits there for its theta (WalkerArgs::arm_*) and starts the moment the host has
                                // pushed it into the launch's slots (device memory, written through the PCIe BAR) -- no launch call, no
                                // command-processor latency, no read over PCIe and none of the kernel's theta-independent entry between the
                                // caller's theta and the arithmetic.  -1: when the previous call came within prearm_us / 2 of the
                                // one before returning (a sampler's loop), 0 never, 1 after every eligible call
    int prearm_us = 500;        // the LONGEST a pre-armed launch waits for its batch before it leaves (the GPU is held meanwhile); the wait it is
                                // actually given follows the caller's rhythm (vp_ctx::Prearm::gap_ema_us): 1.5 x the recent gap between calls + 10 us
    int flux_walker = 1;        // vp_model_flux_batch[_device]: batches the walker kernel would take as lnprob batches as ONE launch (0: prep + tile launches)
    int stretch_mailbox = 1;    // vp_stretch_run's overlapped half-steps (stretch_overlap) keep a walker's row, lnprob and version in one 64-byte
                                // line per buffer where D <= 6 (StretchArgs::ovl = 2); 0 = separate arrays
    int walker_split = 0;       // walker_kernel's split form (WalkerArgs::split: a walker = several workgroups of one-pass tiles): 0 never
                                // (default), N > 0 always N workgroups per walker where the form applies at all, -1 by batch size (eight
                                // where W x 8 workgroups leave every CU at most one: W <= 32 on MI355X).  Measured gain: 15.3 -> 14.0 us
                                // per pass for <= 32 walkers on C1, nothing above (walker_split_for); off by default because it makes a
                                // row's last bit depend on whether its batch has <= 32 rows (one-pass against two-pass tile sums) --
                                // a caller who recomputes a chain's lnprob in one large batch would no longer get the chain's bits
    int slice_seg = 0;          // device slice sampler: iterations per segment (the stretch the device works through without the
                                // host), 0 = as many as the chain chunk and the table of random splits allow (tests: small values)
};

struct Knob { const char* name; const char* env; int is_long; size_t off; };
#define VP_KNOB(field, envname, is_long) {#field, envname, is_long, offsetof(Tuning, field)}
const Knob g_knobs[] = {
    VP_KNOB(prep_rpw, "RBVFIT_AMD_PREP_RPW", 0), VP_KNOB(geom, "RBVFIT_AMD_GEOM", 0),
    VP_KNOB(finalize, "RBVFIT_AMD_FINALIZE", 0), VP_KNOB(walker, "RBVFIT_AMD_WALKER", 0),
    VP_KNOB(zerocopy_max, "RBVFIT_AMD_ZEROCOPY_MAX", 1),
    VP_KNOB(no_zerocopy, "RBVFIT_AMD_NO_ZEROCOPY", 0), VP_KNOB(no_multipole, "RBVFIT_AMD_NO_MULTIPOLE", 0), VP_KNOB(multipole_min, "RBVFIT_AMD_MULTIPOLE_MIN", 0),
    VP_KNOB(span, "RBVFIT_AMD_SPAN", 0), VP_KNOB(waves, "RBVFIT_AMD_WAVES", 0), VP_KNOB(lds_pad, "RBVFIT_AMD_LDS_PAD", 1),
    VP_KNOB(no_fused_accept, "RBVFIT_AMD_NO_FUSED_ACCEPT", 0), VP_KNOB(slice_rows, "RBVFIT_AMD_SLICE_ROWS", 0), VP_KNOB(walker_clusters, "RBVFIT_AMD_WALKER_CLUSTERS", 0), VP_KNOB(no_shared_prep, "RBVFIT_AMD_NO_SHARED_PREP", 0),
    VP_KNOB(farfield, "RBVFIT_AMD_FARFIELD", 0), VP_KNOB(multi_sync, "RBVFIT_AMD_MULTI_SYNC", 0), VP_KNOB(tile_multi, "RBVFIT_AMD_TILE_MULTI", 0), VP_KNOB(no_ff_members, "RBVFIT_AMD_NO_FF_MEMBERS", 0), VP_KNOB(host_spin, "RBVFIT_AMD_HOST_SPIN", 0),
    VP_KNOB(tile_lpt, "RBVFIT_AMD_TILE_LPT", 0), VP_KNOB(gather_plain, "RBVFIT_AMD_GATHER_PLAIN", 0), VP_KNOB(slice_seg, "RBVFIT_AMD_SLICE_SEG", 0),
    VP_KNOB(flux_farfield, "RBVFIT_AMD_FLUX_FARFIELD", 0), VP_KNOB(stretch_overlap, "RBVFIT_AMD_STRETCH_OVERLAP", 0), VP_KNOB(stretch_mailbox, "RBVFIT_AMD_STRETCH_MAILBOX", 0), VP_KNOB(flux_walker, "RBVFIT_AMD_FLUX_WALKER", 0), VP_KNOB(walker_perm, "RBVFIT_AMD_WALKER_PERM", 0), VP_KNOB(walker_prio, "RBVFIT_AMD_WALKER_PRIO", 0), VP_KNOB(walker_perm_hex, "RBVFIT_AMD_WALKER_PERM_HEX", 1),
    VP_KNOB(prearm, "RBVFIT_AMD_PREARM", 0), VP_KNOB(prearm_us, "RBVFIT_AMD_PREARM_US", 0), VP_KNOB(walker_split, "RBVFIT_AMD_WALKER_SPLIT", 0),
};
void set_knob(Tuning& t, const Knob& k, long v) {
    char* base = reinterpret_cast<char*>(&t) + k.off;
    if (k.is_long) *reinterpret_cast<long*>(base) = v; else *reinterpret_cast<int*>(base) = (int)v;
}
Tuning tuning_from_env() {
    Tuning t;
    for (const Knob& k : g_knobs)
        if (const char* e = getenv(k.env))      // set but empty counts as 1; decimal ("010" is ten), hexadecimal for the explicit tile deal alone
            set_knob(t, k, *e ? (std::strcmp(k.name, "walker_perm_hex") == 0 ? (long)strtoull(e, nullptr, 16) : strtol(e, nullptr, 10)) : 1);
    return t;
}

struct Instrument {
    vp::InstDev dev{};
    vp::InstDev dev_s{};         // same instrument, one-pass tiles: used for small batches (lnprob only)
    vp::InstDev dev_w{};         // walker_kernel's geometry: single-wave tiles of 384 evaluated pixels whatever the LSF
                                 // length (= dev for K <= 33; longer LSFs: more halo per tile, but one launch)
    size_t lds_w = 0;            // LDS bytes of one such tile; 0: the LSF is too long for single-wave tiles
    size_t lds_s = 0;            // LDS bytes of one single-wave ONE-pass tile (dev_s where nwaves == 1): walker_kernel's split form; 0: none
    int* split_hint = nullptr;   // (dev_s.ntiles) the split form's "tile met line cores before" hints (InstDev::core_hint of that launch)
    unsigned long long wperm = 0xFEDCBA9876543210ull;   // walker_kernel (this instrument alone): tile of wave k in nibble k (WalkerArgs)
    unsigned long long wperm_shared = 0xFEDCBA9876543210ull; // ... for batches of more than one workgroup per CU (walker_deal_for)
    int deal_ntask = 0;          // waves with entry tasks (they hold the cheapest tiles of both deals) and the tiles' estimated cost:
    std::vector<long> deal_cost; // what the deals were made from (vp_walker_deals)

    vp::LinesDev lines{};
    double sum_logw = 0.0;
    std::vector<void*> allocs;   // device allocations owned by this instrument
    double* d_flux = nullptr;
    double* d_w = nullptr;
    size_t lds_bytes = 0;
    // host copies for the "can any in-bounds walker leave the fast domain?" analysis
    std::vector<double> h_lambda0, h_gamma;
    std::vector<int> h_bidx;
    bool needs_generic = true;
    bool nanfix = false;         // astropy-branch LSF and NaN samples in the wavelength grid: InstDev::rbot (tile launches' NANFIX instances)
    int nwaves = 1;              // waves per tile workgroup (1, 2 or 4)
    bool ff_on = false;          // far-field expansions (farfield_kernel + the FF instance of tile_kernel) for lnprob
    double ff_cover = 0.0;       // estimated share of (block, line) pairs the expansions cover (host, prior-box centre)
    int ff_items = 0;            // multipole clusters + lines outside clusters: what a pass of the tile kernel walks
    std::vector<double> h_lines; // lambda0 | gamma | f | zfac: with h_idx, what the line records of a walker depend on
    std::vector<int> h_idx;      // N_idx | b_idx | v_idx | method | multipole settings
    unsigned long long member_mask[2] = {0ull, 0ull};   // lines that are members of multipole clusters (L <= 128: what the
                                       // far-field masks are compared with, vp_last_farfield_info)
    bool same_lines_as_prev = false;   // this instrument's records ARE the previous instrument's (same line tables):
                                       // its record-preparation launch is skipped (C3: two instruments, one physics)
    int* fisher_off = nullptr;         // (D + 1) fisher_rows_kernel: where the terms of theta index k start in fisher_terms
    int2* fisher_terms = nullptr;      // (3 L) (line, kind) by theta index, then line, then kind; made at the first Fisher / Jacobian call
};

}  // namespace

struct vp_ctx {
    int device = 0;
    pid_t pid = 0;               // the process that created the context (a forked child must not touch its mappings: prearm_leave_all_at_exit)
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;        // vp_stretch_run's overlapped half-steps: the odd half-steps (made on first use)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int num_cus = 0;
    mutable std::mutex mu;
    mutable std::string err;
    Tuning tune;
    size_t lds_limit = 65536;    // dynamic LDS a workgroup may ask for on this device
    int D = 0;
    double* d_lb = nullptr;
    double* d_ub = nullptr;
    std::vector<Instrument> inst;
    // per-batch workspace (grown on demand)
    int capW = 0;
    int capL = 0;          // max records per walker (lines + multipole clusters) the workspace was sized for
    int cap_tiles = 0;
    double* d_theta = nullptr;   // (capW, D)
    double* d_out = nullptr;     // (capW)
    double* d_lc = nullptr;      // (capW, capL, LC_STRIDE)
    double* d_partial = nullptr; // (capW, total_tiles)
    int* d_flags = nullptr;      // (capW)
    unsigned int* d_ticket = nullptr;  // (capW) arrival counters of the fused final reduction
    int* d_genflag = nullptr;    // 2 x (capW) walkers with lines outside the fast domain (per instrument pass): two buffers in turn -- the
                                 // record-preparation launch that fills one clears the other for the launch after it (genflag_acquire)
    unsigned gen_seq = 0;
    int gen_clean[2] = {0, 0};   // leading entries of each buffer known to be zero
    int* h_gen_any = nullptr;    // mapped host memory, one word: has any launch of this context (with these bounds and instruments) flagged a
    int* h_gen_any_dev = nullptr;   // walker?  (what the generic launches are sized by: tile_generic_kernel's grid)
    double* d_ff = nullptr;      // (capW x cap_ffblk, FF_STRIDE) far-field expansions, instrument after instrument
    int cap_ffblk = 0;
    std::vector<double> h_lb;    // host copy of the lower bounds
    std::vector<double> h_ub;    // ... and of the upper bounds
    int* d_tile_off = nullptr;   // 2 x (n_inst + 1): tile offsets of the full-size and of the one-pass geometry
    double* d_sum_logw = nullptr;
    bool meta_dirty = true;
    int total_tiles = 0;         // max over the two geometries (workspace size)
    int total_tiles_g[2] = {0, 0};
    int total_tiles_w = 0;       // tiles of all instruments in the single-wave geometry (tile_kernel_multi)
    double* h_pinned = nullptr;  // staging for theta / out
    double* h_pinned_dev = nullptr;   // ... as the device sees it (zero-copy batches)
    size_t h_pinned_bytes = 0;
    // completion of a host-buffer call without an interrupt: the stream writes a sequence number to a host-mapped word
    // behind the batch (hipStreamWriteValue32), the calling thread spins on it (host_wait)
    uint32_t* h_done = nullptr;
    uint32_t done_seq = 0;
    bool done_armed = false;     // the last batch enqueued carries a completion write
    // host_spin = 2: the last batch's output rows are what the host polls (lnprob_host_begin / host_wait)
    bool sentinel_armed = false;
    int sentinel_W = 0;
    const double* sentinel_out = nullptr;
    // pre-armed launch of the next vp_lnprob_batch call (Tuning::prearm)
    struct Prearm {
        uint32_t* h = nullptr;        // pinned host block the LAUNCH writes: h[16] "expired", h[32] "stuck"
        uint32_t* h_dev = nullptr;    // ... as the device sees it
        int bar = -1;                 // can the CPU write device memory (large BAR)?  -1 not asked yet
        double* slots = nullptr;      // fine-grained device memory the CPU writes through the BAR: slot_doubles per row (WalkerArgs::arm_slots)
        int slot_doubles = 0, slot_rows = 0;
        const double* theta_src = nullptr;    // the caller's theta of the batch in flight (only the slots have it so far)
        bool live = false;            // a launch is waiting on the stream (or has expired there)
        bool dirty = false;           // a pre-armed launch has been put on live_stream since the last fence: it writes rehearsal records into the
                                      // shared workspace even when it is sent away, so work on ANOTHER stream must be ordered behind it (foreign_stream_fence)
        hipEvent_t ev = nullptr;
        uint32_t seq = 0;             // ... with this sequence number
        int W = 0;                    // ... for this many rows
        hipStream_t cur = nullptr;    // the stream of the launch that serves the current call
        hipStream_t live_stream = nullptr;    // the stream the waiting launch is on
        bool inflight = false;        // the batch host_wait is waiting for was started through a pre-armed launch (seq_inflight)
        uint32_t seq_inflight = 0;
        bool have_last = false;       // last_return is set
        int last_W = -1;              // rows of the previous vp_lnprob_batch call
        std::chrono::steady_clock::time_point last_return;
        int misses = 0;               // consecutive launches that expired although their batch had been pushed
        // being a good neighbour: a waiting launch holds every CU, and only this library's own entry points can send it away --
        // anything else the process (or another process) puts on the GPU waits it out.  So it waits no longer than the caller's
        // own rhythm suggests, and a caller whose launches expire unused is left alone for a while.
        double gap_ema_us = 0.0;      // running mean of the time between a call's return and the next call (calls that came within prearm_us)
        int budget_us = 0;            // how long the launch now waiting was told to wait
        int cooldown = 0;             // calls still to pass before the next launch is pre-armed (set when one expired unused)
        int cooldown_next = 8;        // ... and what the next unused expiry will set it to (doubles, back to 8 after 16 used in a row)
        int used_streak = 0;
        int64_t used = 0, expired = 0, cancelled = 0;     // (vp_prearm_counts)
    } arm;
    bool sentinel_unsafe = false;    // some static input (bounds, spectra, line tables, taps) carries the sentinel's NaN payload
    // direct-write gather of the lnprob vector between the ranks of a multi-process job (vp_gather_*)
    struct Gather {
        int W = 0, world = 0, rank = 0, seq = 0;
        bool connected = false, finegrained = false;
        bool local_peers = false;              // the peers' vectors are plain device pointers of contexts of this process (no IPC mapping to close)
        bool shared_device = false;            // some ranks share a GPU: the handshake is a launch of its own (replicas_handshake)
        double* buf = nullptr;                 // (world, W) this rank's gathered vector
        int* flags = nullptr;                  // (MAX_REPLICAS) flags[r] = the last pass whose block from rank r has landed here
        unsigned int* done = nullptr;          // workgroup counters of the running launch (PUB_GROUPS + 1) | timeout flag (int)
        double* peer_buf[vp::MAX_REPLICAS] = {};
        int* peer_flags[vp::MAX_REPLICAS] = {};
    } gather;
    const vp::Replicas* gather_rep = nullptr;   // set around an enqueue_lnprob whose results go into the ranks' gathered vectors
    // workspace of the gradient path (vp_lnprob_grad_batch*, capi_grad.inc), grown on demand; sizes in doubles
    struct Grad {
        double* fl = nullptr;     // (rows, P) unconvolved flux, then s = d lnL / d tau_total
        double* q = nullptr;      // (rows, P) d lnL / d model
        double* rec = nullptr;    // (rows, L, LC_STRIDE) line records
        double* part = nullptr;   // (rows, L, chunks, 3) partial sums of the lines
        double* io = nullptr;     // host entry: theta | grad | lnprob
        size_t n_fl = 0, n_q = 0, n_rec = 0, n_part = 0, n_io = 0;
    } grad;
    // ... and what the Jacobian / Fisher path adds to it (vp_model_flux_jacobian, vp_fisher_batch*, capi_fisher.inc)
    struct Fisher {
        double* g = nullptr;      // (rows, D, P) derivative rows before the LSF
        double* J = nullptr;      // (rows, D, P) d model_flux / d theta
        double* part = nullptr;   // (rows, chunks, D, D) partial Fisher blocks (upper triangles)
        double* io = nullptr;     // host entries: theta | lnprob | fisher
        size_t n_g = 0, n_J = 0, n_part = 0, n_io = 0;
    } fisher;
    // model_flux / voigt_h scratch
    double* d_scratch = nullptr;
    size_t scratch_bytes = 0;
    // optional per-kernel timing with HIP events on the launch stream (bench.py roofline leg)
    int last_kind = 0;           // launch structure of the last lnprob batch: 0 prep + tile (+ finalize), 1 walker_kernel
    int last_split = 0;          // ... and, for walker_kernel, the workgroups per walker of its split form (0: the ordinary form)
    // the far-field expansions the last lnprob batch made for its FIRST instrument that took any (vp_last_farfield_info):
    // where they lie in the workspace, rows, blocks per row, which farfield_kernel instance, which instrument
    struct LastFF { const double* ff = nullptr; int W = 0, nbk = 0, members = 0, inst = -1; } last_ff;
    bool profiling = false;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    struct Span { size_t a, b; int kind; };   // kind: 0 prep, 1 tile, 2 finalize
    std::vector<Span> spans;
};

struct vp_multi {
    std::vector<vp_ctx*> ctx;
    std::mutex mu;
    std::string err;
    bool no_peer = false;        // some pair of devices cannot map each other's memory: no sharded device-resident sampler
    std::vector<hipEvent_t> ev;  // one per context: the half-step barrier of vp_multi_stretch_run
    bool broken = false;         // a setup call failed half-way and could not be undone: the contexts differ, every later call fails
};

namespace {

int fail(const vp_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

#define HIP_TRY(c, expr)                                                                     \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess)                                                               \
            return fail((c), VP_EHIP, std::string(#expr) + ": " + hipGetErrorString(e__));   \
    } while (0)

// (pad: zeroed elements behind the n uploaded ones -- the observed spectrum and its weights are read six pixels per lane with
//  16-byte loads, lsf_block6, and a lane past the end of the last tile reads up to eight doubles beyond the array)
template <class T>
int upload(vp_ctx* c, Instrument* ins, const T* host, size_t n, T** out, size_t pad = 0) {
    T* d = nullptr;
    HIP_TRY(c, hipMalloc((void**)&d, ((n ? n : 1) + pad) * sizeof(T)));
    if (ins) ins->allocs.push_back(d);
    if (pad) HIP_TRY(c, hipMemset(d + n, 0, pad * sizeof(T)));
    if (n) HIP_TRY(c, hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice));
    *out = d;
    return VP_OK;
}

double neumaier_sum(const double* v, int n) {
    double s = 0.0, comp = 0.0;
    for (int i = 0; i < n; ++i) {
        double t = s + v[i];
        if (std::fabs(s) >= std::fabs(v[i])) comp += (s - t) + v[i]; else comp += (v[i] - t) + s;
        s = t;
    }
    return s + comp;
}

// The NaN the output rows of a zero-copy host batch are pre-set to (host_spin = 2).  Hardware-made NaNs are the default quiet NaN
// and NaN inputs travel through arithmetic with their payload (quieted, sign possibly flipped): an output can only equal
// the pattern if an INPUT carried this payload, and every entry point that takes doubles looks for it.
constexpr uint64_t VP_SENTINEL_BITS = 0x7FF8A5C3965A3C69ull;
inline bool carries_sentinel(const double* v, size_t n) {
    bool hit = false;
    for (size_t i = 0; i < n; ++i) {
        uint64_t b;
        std::memcpy(&b, v + i, 8);
        hit |= ((b & 0x7FFFFFFFFFFFFFFFull) | 0x0008000000000000ull) == VP_SENTINEL_BITS;
    }
    return hit;
}

int ensure_scratch(vp_ctx* c, size_t bytes) {
    if (bytes <= c->scratch_bytes) return VP_OK;
    if (c->d_scratch) HIP_TRY(c, hipFree(c->d_scratch));
    c->d_scratch = nullptr; c->scratch_bytes = 0;
    HIP_TRY(c, hipMalloc((void**)&c->d_scratch, bytes));
    c->scratch_bytes = bytes;
    return VP_OK;
}

// Bump allocator over a buffer.  An entry point that cuts d_scratch into sub-buffers states its layout ONCE, as a function that
// fills its Dev struct from an Arena (carve_scratch): run over a null base it measures, run over d_scratch it carves -- no size
// formula beside the pointers.  (hipMalloc's alignment exceeds any asked for here, so both runs pad alike.)
struct Arena {
    uintptr_t at;
    explicit Arena(void* p = nullptr) : at(reinterpret_cast<uintptr_t>(p)) {}
    template <class T> T* take(size_t count, size_t align = alignof(T)) {
        T* p = reinterpret_cast<T*>(at = (at + align - 1) & ~(uintptr_t)(align - 1));
        at += count * sizeof(T);
        return p;
    }
    size_t bytes_from(const void* p) const { return at - reinterpret_cast<uintptr_t>(p); }   // from a sub-buffer taken earlier to here
};
template <class Layout> int carve_scratch(vp_ctx* c, Layout layout) {
    Arena measure;
    layout(measure);                                  // (what it fills now is overwritten below)
    if (int rc = ensure_scratch(c, measure.bytes_from(nullptr))) return rc;
    Arena a(c->d_scratch);
    layout(a);
    return VP_OK;
}

// rows [lo, lo + n) of n_total that context i of several works on: contiguous blocks of `per` rows, the last ones short or empty
std::pair<int, int> block_of(int i, int per, int n_total) { const int lo = std::min(i * per, n_total); return {lo, std::min(lo + per, n_total) - lo}; }
// steps of a stretch run's chain kept on the device between two copies to the host: 256 MiB worth of rows, at least one
size_t chain_chunk(int nsteps, size_t row_doubles) {
    return std::max<size_t>(1, std::min<size_t>((size_t)std::max(nsteps, 1), ((size_t)256 << 20) / (row_doubles * sizeof(double))));
}

int ensure_pinned(vp_ctx* c, size_t bytes) {
    if (bytes <= c->h_pinned_bytes) return VP_OK;
    if (c->h_pinned) HIP_TRY(c, hipHostFree(c->h_pinned));
    c->h_pinned = nullptr; c->h_pinned_bytes = 0; c->h_pinned_dev = nullptr;
    HIP_TRY(c, hipHostMalloc((void**)&c->h_pinned, bytes, hipHostMallocDefault));
    c->h_pinned_bytes = bytes;
    return VP_OK;
}

int ensure_workspace(vp_ctx* c, int W) {
    int maxL = 1;
    for (auto& in : c->inst) maxL = std::max(maxL, in.dev.L + in.dev.NCm);
    if (c->meta_dirty) {
        const size_t n1 = c->inst.size() + 1;
        std::vector<int> off(3 * n1, 0);                   // full-size | one-pass | single-wave (dev_w) geometry
        std::vector<double> slw(n1, 0.0);
        for (size_t k = 0; k < c->inst.size(); ++k) {
            off[k + 1] = off[k] + c->inst[k].dev.ntiles;
            off[n1 + k + 1] = off[n1 + k] + c->inst[k].dev_s.ntiles;
            off[2 * n1 + k + 1] = off[2 * n1 + k] + c->inst[k].dev_w.ntiles;
            slw[k] = c->inst[k].sum_logw;
        }
        c->total_tiles_g[0] = off[n1 - 1];
        c->total_tiles_g[1] = off[2 * n1 - 1];
        c->total_tiles_w = off[3 * n1 - 1];
        c->total_tiles = std::max({c->total_tiles_g[0], c->total_tiles_g[1], c->total_tiles_w});
        if (c->d_tile_off) HIP_TRY(c, hipFree(c->d_tile_off));
        if (c->d_sum_logw) HIP_TRY(c, hipFree(c->d_sum_logw));
        HIP_TRY(c, hipMalloc((void**)&c->d_tile_off, off.size() * sizeof(int)));
        HIP_TRY(c, hipMalloc((void**)&c->d_sum_logw, slw.size() * sizeof(double)));
        HIP_TRY(c, hipMemcpy(c->d_tile_off, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(c->d_sum_logw, slw.data(), slw.size() * sizeof(double), hipMemcpyHostToDevice));
        c->meta_dirty = false;
    }
    int ffblk = 0;
    for (auto& in : c->inst)
        if (in.ff_on) ffblk += std::max(in.dev.ntiles * in.dev.ff_nblk, in.dev_s.ntiles * in.dev_s.ff_nblk);   // (every instrument its own stretch)
    if (W <= c->capW && maxL <= c->capL && c->total_tiles <= c->cap_tiles && ffblk <= c->cap_ffblk) return VP_OK;
    // a stream-ordered previous call may still be using the old buffers
    HIP_TRY(c, hipDeviceSynchronize());
    const int newW = std::max(W, c->capW);
    for (void* p : {(void*)c->d_theta, (void*)c->d_out, (void*)c->d_lc, (void*)c->d_partial, (void*)c->d_flags, (void*)c->d_ticket, (void*)c->d_genflag,
                    (void*)c->d_ff})
        if (p) HIP_TRY(c, hipFree(p));
    c->d_theta = c->d_out = c->d_lc = c->d_partial = nullptr; c->d_flags = nullptr; c->d_ticket = nullptr; c->d_genflag = nullptr; c->capW = 0;
    c->d_ff = nullptr; c->cap_ffblk = 0;
    if (ffblk > 0) HIP_TRY(c, hipMalloc((void**)&c->d_ff, (size_t)newW * ffblk * vp::FF_STRIDE * sizeof(double)));
    HIP_TRY(c, hipMalloc((void**)&c->d_theta, (size_t)newW * std::max(c->D, 1) * sizeof(double)));
    HIP_TRY(c, hipMalloc((void**)&c->d_out, (size_t)newW * sizeof(double)));
    // (at least 1024 rows of records: walker_kernel's split form gives every workgroup of a walker its own rows -- W x split <= 512 --
    //  and the stretch sampler keeps two half-steps in flight)
    HIP_TRY(c, hipMalloc((void**)&c->d_lc, (size_t)std::max(newW, 1024) * maxL * vp::LC_STRIDE * sizeof(double)));
    HIP_TRY(c, hipMalloc((void**)&c->d_partial, (size_t)newW * std::max(c->total_tiles, 1) * sizeof(double)));
    HIP_TRY(c, hipMalloc((void**)&c->d_flags, (size_t)newW * sizeof(int)));
    HIP_TRY(c, hipMemset(c->d_flags, 0, (size_t)newW * sizeof(int)));
    HIP_TRY(c, hipMalloc((void**)&c->d_ticket, (size_t)newW * sizeof(unsigned int)));
    HIP_TRY(c, hipMemset(c->d_ticket, 0, (size_t)newW * sizeof(unsigned int)));
    HIP_TRY(c, hipMalloc((void**)&c->d_genflag, 2 * (size_t)newW * sizeof(int)));
    HIP_TRY(c, hipMemset(c->d_genflag, 0, 2 * (size_t)newW * sizeof(int)));
    c->gen_clean[0] = c->gen_clean[1] = newW;
    c->capW = newW; c->capL = maxL; c->cap_tiles = c->total_tiles; c->cap_ffblk = ffblk;
    return VP_OK;
}

