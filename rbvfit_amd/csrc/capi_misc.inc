// capi_misc.inc -- entry points: Philox hook, H(a,x) test hook, per-kernel timing, introspection.
// A fragment of the ONE translation unit capi.hip (included there inside extern "C", in order; not a header of its own).
void vp_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    const vp::Philox4 r = vp::philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    for (int i = 0; i < 4; ++i) out[i] = r.v[i];
}

int vp_voigt_h(vp_ctx* c, int na, const double* a, int nx, const double* x, double* out) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    if (na <= 0 || nx <= 0 || !a || !x || !out) return fail(c, VP_EINVAL, "vp_voigt_h: empty or NULL input");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t rec = (size_t)na * vp::LC_STRIDE, need = (rec + na + nx + (size_t)na * nx) * sizeof(double);
    int rc;
    if ((rc = ensure_scratch(c, need))) return rc;
    double* d_rec = c->d_scratch;
    double* d_a = d_rec + rec;
    double* d_x = d_a + na;
    double* d_o = d_x + nx;
    HIP_TRY(c, hipMemcpyAsync(d_a, a, na * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_x, x, nx * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(vp::prep_h_kernel, dim3((na + 63) / 64), dim3(64), 0, c->stream, d_a, (int)na, d_rec);
    hipLaunchKernelGGL(vp::voigt_h_kernel, dim3((nx + 255) / 256, na), dim3(256), 0, c->stream, d_rec, d_x, nx, d_o);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, d_o, (size_t)na * nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return VP_OK;
}

int vp_profile_enable(vp_ctx* c, int enable) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    c->profiling = enable != 0;
    c->ev_used = 0;
    c->spans.clear();
    return VP_OK;
}

int vp_profile_read(vp_ctx* c, double* prep_ms, double* tile_ms, double* finalize_ms, int* n_tile_launches) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    HIP_TRY(c, hipSetDevice(c->device));
    double acc[3] = {0, 0, 0};
    int ntile = 0;
    for (const auto& sp : c->spans) {
        if (sp.a == (size_t)-1 || sp.b == (size_t)-1) continue;
        HIP_TRY(c, hipEventSynchronize(c->ev_pool[sp.b]));
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_pool[sp.a], c->ev_pool[sp.b]));
        acc[sp.kind] += ms;
        if (sp.kind == 1) ++ntile;
    }
    if (prep_ms) *prep_ms = acc[0];
    if (tile_ms) *tile_ms = acc[1];
    if (finalize_ms) *finalize_ms = acc[2];
    if (n_tile_launches) *n_tile_launches = ntile;
    c->ev_used = 0;
    c->spans.clear();
    return VP_OK;
}


int vp_num_instruments(const vp_ctx* c) {
    if (!c) return 0;
    std::lock_guard<std::mutex> g(c->mu);
    return (int)c->inst.size();
}
int vp_ndim(const vp_ctx* c) {
    if (!c) return 0;
    std::lock_guard<std::mutex> g(c->mu);
    return c->D;
}
int vp_instrument_pixels(const vp_ctx* c, int inst) {
    if (!c) return -1;
    std::lock_guard<std::mutex> g(c->mu);
    if (inst < 0 || inst >= (int)c->inst.size()) return -1;
    return c->inst[inst].dev.P;
}
int vp_device_id(const vp_ctx* c) { return c ? c->device : -1; }
int vp_last_farfield_info(vp_ctx* c, int* variant, int64_t* covered, int64_t* covered_members, int64_t* pairs) {
    if (!c) return VP_EINVAL;
    CtxGuard g(c);
    if (variant) *variant = 0;
    if (covered) *covered = 0;
    if (covered_members) *covered_members = 0;
    if (pairs) *pairs = 0;
    const vp_ctx::LastFF lf = c->last_ff;
    if (lf.inst < 0 || !lf.ff || lf.W <= 0 || lf.nbk <= 0) return VP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize());
    const size_t n = (size_t)lf.W * lf.nbk;
    std::vector<double> h(n * vp::FF_STRIDE);
    HIP_TRY(c, hipMemcpy(h.data(), lf.ff, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    const Instrument& in = c->inst[lf.inst];
    int64_t cov = 0, mem = 0;
    for (size_t i = 0; i < n; ++i) {
        unsigned long long m[2];
        memcpy(m, h.data() + i * vp::FF_STRIDE + vp::FF_MASK0, sizeof m);
        cov += __builtin_popcountll(m[0]) + __builtin_popcountll(m[1]);
        mem += __builtin_popcountll(m[0] & in.member_mask[0]) + __builtin_popcountll(m[1] & in.member_mask[1]);
    }
    if (variant) *variant = lf.members ? 2 : 1;
    if (covered) *covered = cov;
    if (covered_members) *covered_members = mem;
    if (pairs) *pairs = (int64_t)n * in.lines.L;
    return VP_OK;
}

int vp_walker_deals(const vp_ctx* c, int inst, uint64_t deals[2], int64_t* cost, int max_tiles, int* ntiles, int* ntask) {
    if (!c) return VP_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    if (inst < 0 || inst >= (int)c->inst.size()) return VP_EINVAL;
    const Instrument& in = c->inst[inst];
    if (deals) { deals[0] = in.wperm; deals[1] = in.wperm_shared; }
    if (ntiles) *ntiles = in.dev_w.ntiles;
    if (ntask) *ntask = in.deal_ntask;
    for (int t = 0; cost && t < max_tiles; ++t) cost[t] = t < (int)in.deal_cost.size() ? in.deal_cost[t] : 0;
    return VP_OK;
}
int vp_last_launch_kind(const vp_ctx* c) {
    if (!c) return -1;
    std::lock_guard<std::mutex> g(c->mu);
    return c->last_kind;
}
int vp_last_walker_split(const vp_ctx* c) {
    if (!c) return -1;
    std::lock_guard<std::mutex> g(c->mu);
    return c->last_kind == 1 ? c->last_split : 0;
}

