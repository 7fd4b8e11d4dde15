// capi_prearm.inc -- pre-armed launches of the host-buffer entry, the registry of live contexts, argument checks.
// A fragment of the ONE translation unit capi.hip (included there, in order; not a header of its own).
// ---- pre-armed launches (Tuning::prearm, WalkerArgs::arm_*) -------------------------------------------------------------
// (all called with c->mu held)
// what the host writes into the slots (through the BAR: stores only, never a load; the word goes last)
void prearm_push(vp_ctx* c, int W, const double* theta, int code) {
    const int n = c->arm.slot_doubles, D = c->D;
    const uint64_t word = ((uint64_t)c->arm.seq << 2) | (uint64_t)code;
    double* s = c->arm.slots;
    if (!theta) {
        for (int w = 0; w < W; ++w) reinterpret_cast<volatile uint64_t*>(s + (size_t)w * n)[n - 1] = word;
    } else if (n == 8) {
        // one 64-byte line per row: the row, padding, the word -- written in address order, so the write-combining buffer goes out
        // as one burst
        // (no fence between row and word -- it would cut the burst in two --: the word carries a fold of the row's bits in its upper
        //  half and the waiting workgroup takes the row only when it matches, arm_wait)
        for (int w = 0; w < W; ++w) {
            volatile double* q = s + (size_t)w * 8;
            const double* t = theta + (size_t)w * D;
            uint64_t h = 0;
            int k = 0;
            for (; k < D; ++k) { uint64_t b; std::memcpy(&b, t + k, 8); h ^= b; q[k] = t[k]; }
            for (; k < 7; ++k) q[k] = 0.0;
            reinterpret_cast<volatile uint64_t*>(q)[7] = word | ((uint64_t)(uint32_t)(h ^ (h >> 32)) << 32);
        }
    } else {
        for (int w = 0; w < W; ++w) std::memcpy(s + (size_t)w * n, theta + (size_t)w * D, (size_t)D * sizeof(double));
        __builtin_ia32_sfence();            // rows before words (write-combining buffers of different lines go out in any order)
        for (int w = 0; w < W; ++w) reinterpret_cast<volatile uint64_t*>(s + (size_t)w * n)[n - 1] = word;
    }
    __builtin_ia32_sfence();
}
// tell a waiting launch to leave: it has read nothing that depends on a batch and written nothing
void prearm_cancel(vp_ctx* c) {
    if (!c->arm.live) return;
    prearm_push(c, c->arm.W, nullptr, vp::ARM_LEAVE);
    c->arm.live = false;
    ++c->arm.cancelled;
}
// may the NEXT call of this shape be started through a pre-armed launch?
bool prearm_eligible(vp_ctx* c, int W, size_t theta_bytes) {
    return c->tune.prearm != 0 && c->arm.bar != 0 && c->tune.host_spin >= 2 && !c->sentinel_unsafe && !c->gather_rep && !c->profiling &&
           theta_bytes <= (size_t)std::max(0l, c->tune.zerocopy_max) && !c->tune.no_zerocopy && walker_applies(c, W);
}
int prearm_launch(vp_ctx* c, int W) {
    if (c->arm.bar < 0) {
        // device memory the CPU can write: every GPU of this class has its whole memory behind the PCIe BAR; without it there
        // are no pre-armed launches
        int v = 0;
        c->arm.bar = (hipDeviceGetAttribute(&v, hipDeviceAttributeIsLargeBar, c->device) == hipSuccess && v) ? 1 : 0;
        (void)hipGetLastError();
        if (!c->arm.bar) return VP_OK;
    }
    if (!c->arm.h) {
        if (hipHostMalloc((void**)&c->arm.h, 256, hipHostMallocMapped) != hipSuccess) { c->arm.h = nullptr; c->arm.bar = 0; (void)hipGetLastError(); return VP_OK; }
        std::memset(c->arm.h, 0, 256);
        HIP_TRY(c, hipHostGetDevicePointer((void**)&c->arm.h_dev, c->arm.h, 0));
    }
    const int n = 8 * ((c->D + 1 + 7) / 8);
    if (!c->arm.slots || c->arm.slot_rows < W || c->arm.slot_doubles != n) {
        // (no launch is waiting here: a batch of another shape has sent it away -- hipFree waits for it)
        if (c->arm.slots) HIP_TRY(c, hipFree(c->arm.slots));
        c->arm.slots = nullptr;
        const size_t bytes = (size_t)W * n * sizeof(double);
        if (hipExtMallocWithFlags((void**)&c->arm.slots, bytes, hipDeviceMallocFinegrained) != hipSuccess) {
            c->arm.slots = nullptr; c->arm.bar = 0; (void)hipGetLastError(); return VP_OK;
        }
        HIP_TRY(c, hipMemset(c->arm.slots, 0, bytes));
        HIP_TRY(c, hipDeviceSynchronize());
        {   // is the allocation really in this process's address space?  (asked of the kernel, not found out by a fault)
            const uintptr_t pg = (uintptr_t)sysconf(_SC_PAGESIZE), a0 = (uintptr_t)c->arm.slots & ~(pg - 1);
            unsigned char vec[1];
            if (mincore((void*)a0, 1, vec) != 0 && errno == ENOMEM) {
                (void)hipFree(c->arm.slots);
                c->arm.slots = nullptr; c->arm.bar = 0;
                return VP_OK;
            }
        }
        c->arm.slot_rows = W;
        c->arm.slot_doubles = n;
    }
    c->arm.seq = (c->arm.seq + 1) & 0x3fffffffu;
    if (c->arm.seq == 0) c->arm.seq = 1;
    hipStream_t s = c->stream;
    double* dp = c->h_pinned_dev;
    launch_walker(c, plan_lnprob(c, W), W, dp, dp + (size_t)W * c->D, s, true);
    HIP_TRY(c, hipGetLastError());
    c->arm.live = true;
    c->arm.dirty = true;
    c->arm.live_stream = s;
    c->arm.W = W;
    return VP_OK;
}
// An entry point about to enqueue on a stream of the caller's: a pre-armed launch -- waiting, sent away or expired -- may still be
// writing its rehearsal records into the context's record workspace on the context's own stream; order the caller's stream behind it.
int foreign_stream_fence(vp_ctx* c, hipStream_t s) {
    if (!c->arm.dirty || !c->arm.live_stream || s == c->arm.live_stream) return VP_OK;       // (same stream: stream order does it)
    if (!c->arm.ev) HIP_TRY(c, hipEventCreateWithFlags(&c->arm.ev, hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(c->arm.ev, c->arm.live_stream));
    HIP_TRY(c, hipStreamWaitEvent(s, c->arm.ev, 0));
    c->arm.dirty = false;
    return VP_OK;
}
// Contexts alive in this process: a program that ends without vp_ctx_destroy must not leave a launch waiting on the GPU while the
// runtime is taken down under it -- at exit every waiting launch is told to leave (CPU stores into its slots, no HIP call).
std::mutex g_ctx_mu;
std::vector<vp_ctx*> g_ctxs;
void prearm_leave_all_at_exit() {
    std::lock_guard<std::mutex> g(g_ctx_mu);
    bool any = false;
    const pid_t me = getpid();
    for (vp_ctx* c : g_ctxs)
        // (a forked child that leaves through exit() runs this handler too: the parent's device mappings are not in its address
        //  space -- ROCm marks them MADV_DONTFORK -- and the launch is the parent's to send away)
        if (c->pid == me && c->mu.try_lock()) {
            any |= c->arm.live;
            prearm_cancel(c);
            c->mu.unlock();
        }
    if (any) std::this_thread::sleep_for(std::chrono::microseconds(100));      // (a workgroup polls its slot every ~0.5 us)
}
void ctx_register(vp_ctx* c) {
    std::lock_guard<std::mutex> g(g_ctx_mu);
    static bool hooked = false;
    if (!hooked) { std::atexit(prearm_leave_all_at_exit); hooked = true; }     // (behind the HIP runtime's own handlers: runs before them)
    c->pid = getpid();
    g_ctxs.push_back(c);
}
void ctx_unregister(vp_ctx* c) {
    std::lock_guard<std::mutex> g(g_ctx_mu);
    g_ctxs.erase(std::remove(g_ctxs.begin(), g_ctxs.end(), c), g_ctxs.end());
}
// A launch that waits holds its compute units: work of ANOTHER context of this process on the same GPU would sit behind it until it
// expires.  Every entry point therefore sends the other contexts' waiting launches away first (one short lock when there are none).
void prearm_cancel_others(vp_ctx* c) {
    std::lock_guard<std::mutex> g(g_ctx_mu);
    if (g_ctxs.size() < 2) return;
    for (vp_ctx* o : g_ctxs)
        if (o != c && o->device == c->device && o->mu.try_lock()) {       // (a context busy in a call of its own has no launch waiting)
            prearm_cancel(o);
            o->mu.unlock();
        }
}
struct CtxGuard {                 // every entry but vp_lnprob_batch itself: lock the context and send a waiting launch away
    std::lock_guard<std::mutex> g;
    explicit CtxGuard(vp_ctx* c) : g(c->mu) { prearm_cancel(c); prearm_cancel_others(c); }
};

// (called with c->mu held)
int check_batch_args(vp_ctx* c, int W, int D, const void* a, const void* b) {
    if (c->D <= 0) return fail(c, VP_ESTATE, "vp_set_bounds has not been called");
    if (c->inst.empty()) return fail(c, VP_ESTATE, "no instrument has been added");
    if (D != c->D) return fail(c, VP_EINVAL, "theta has D=" + std::to_string(D) + " but the context was set up with D=" + std::to_string(c->D));
    if (W < 0) return fail(c, VP_EINVAL, "negative batch size");
    if (W > 0 && (!a || !b)) return fail(c, VP_EINVAL, "NULL theta/out");
    return VP_OK;
}

}  // namespace
