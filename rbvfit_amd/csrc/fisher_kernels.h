// Model Jacobian and Fisher matrix (vp_model_flux_jacobian, vp_fisher_batch*): fp64, per walker row, no atomics.
//
//     g_k[p] = -fl[p] sum_{(l, kind) : idx(l, kind) = k} d tau_lp / d (logN | b | v)_l      (derivative rows; tied parameters fold here)
//     J_k    = LSF(g_k) = d model_flux / d theta_k                                          (edge-replicated taps, as grad_q_kernel)
//     F_jk   = sum_inst sum_p w_p J_j[p] J_k[p]                                             (j <= k, mirrored on write)
//
// Launches per instrument and pass of rows, all on one stream: grad_prep_kernel and grad_flux_kernel (grad_kernels.h, unchanged:
// line records and fl), fisher_rows_kernel (one workgroup per (256 pixels, theta index, walker): the per-pixel derivatives are
// those grad_lines_kernel forms from dw_line, summed over the (line, kind) terms tied to the index, in line order -- the host
// lists them once per instrument, no kernel searches), fisher_conv_kernel (row tile + halo staged in LDS once, K taps read from
// there), fisher_block_kernel (one workgroup per (pixel chunk, 32 x 32 tile pair of F, walker): the rows of the two tiles staged
// pixel-major in LDS, 4 x 4 accumulators per lane, the four waves' pixel slices added in wave order), fisher_reduce_kernel
// (chunks in order; instruments add in launch order).  A row's bits depend on that row and the instrument tables alone.
//
// Rows whose lnprob is not finite get a NaN (D, D) block (grad_init_kernel with D x D columns); every kernel leaves at once for
// such a row.
#pragma once
#include "grad_kernels.h"

namespace vp {

constexpr int FISHER_CONV_PX = 8;                                   // outputs per lane of fisher_conv_kernel
constexpr int FISHER_CONV_TILE = GRAD_THREADS * FISHER_CONV_PX;      // outputs per workgroup: 2048 (+ K - 1 <= 2048 halo pixels in LDS)
constexpr int FISHER_TILE = 32;                                      // rows of F per tile
constexpr int FISHER_PXT = 64;                                       // pixels staged at a time (16 per wave)
constexpr int FISHER_LDS_STRIDE = 2 * FISHER_TILE + 2;               // doubles per staged pixel: 16-byte aligned, rows of a pixel spread over the banks
constexpr int FISHER_CHUNK = 512;                                    // pixels per workgroup of fisher_block_kernel

// g[w][k][p] for every theta index k.  terms[off[k] .. off[k + 1]) = (line, kind) pairs tied to k, by line then kind
// (kind 0 logN, 1 b, 2 v); an index no line of this instrument carries gets a row of zeros.
__global__ __launch_bounds__(GRAD_THREADS) void fisher_rows_kernel(InstDev I, const double* __restrict__ rec, const double* __restrict__ lnprob,
                                                                   const double* __restrict__ fl, const int* __restrict__ off,
                                                                   const int2* __restrict__ terms, int D, double* __restrict__ g) {
    const int k = blockIdx.y, w = blockIdx.z;
    if (!grad_row_valid(lnprob, w)) return;
    const int p = blockIdx.x * GRAD_THREADS + threadIdx.x;
    const int pc = min(p, I.P - 1);                       // (every lane stays active: the tiers are chosen by ballot)
    const double wv = I.wave[pc], gi = I.ginv[pc];
    double acc = 0.0;
    const int t1 = off[k + 1];
    for (int t = off[k]; t < t1; ++t) {                   // (workgroup-uniform)
        const int2 lk = terms[t];
        rec_t r = as_rec(rec + ((size_t)w * I.L + lk.x) * LC_STRIDE);
        const int mode = rec_int(r, LC_MODE, 0), nodd = rec_int(r, LC_MODE, 1);
        const double a = r[LC_Y], T = r[LC_T];
        const double x = faithful_x(wv, gi, r);
        const DW h = dw_line(x, a, ea2_small(a), mode, nodd);
        double d;
        if (lk.y == 0) d = LN10 * (T * h.H);
        else if (lk.y == 1) d = -(T * r[GR_IB]) * h.G;
        else d = T * h.Hx * ((x + r[LC_B]) * r[GR_RCV]);
        acc += d;
    }
    if (p < I.P) g[((size_t)w * D + k) * I.P + p] = -fl[(size_t)w * I.P + p] * acc;
}

// J[w][k][p] = sum_j kflip[j] g[w][k][clamp(p - halo_lo + j)].  Dynamic LDS: (FISHER_CONV_TILE + K - 1) doubles.
__global__ __launch_bounds__(GRAD_THREADS) void fisher_conv_kernel(InstDev I, const double* __restrict__ lnprob, const double* __restrict__ g,
                                                                   int D, double* __restrict__ J) {
    extern __shared__ double fisher_conv_lds[];
    const int k = blockIdx.y, w = blockIdx.z;
    if (!grad_row_valid(lnprob, w)) return;
    const int p0 = blockIdx.x * FISHER_CONV_TILE;
    const int nout = min(FISHER_CONV_TILE, I.P - p0);
    const double* __restrict__ row = g + ((size_t)w * D + k) * I.P;
    const int nstage = nout + I.K - 1;
    for (int i = threadIdx.x; i < nstage; i += GRAD_THREADS)
        fisher_conv_lds[i] = row[min(max(p0 - I.halo_lo + i, 0), I.P - 1)];
    // (lanes past nout read staged-or-stale words below and never store; keep their reads inside the allocation)
    for (int i = nstage + (int)threadIdx.x; i < FISHER_CONV_TILE + I.K - 1; i += GRAD_THREADS) fisher_conv_lds[i] = 0.0;
    __syncthreads();
    double acc[FISHER_CONV_PX];
#pragma unroll
    for (int r = 0; r < FISHER_CONV_PX; ++r) acc[r] = 0.0;
    for (int j = 0; j < I.K; ++j) {
        const double kj = I.kflip[j];
#pragma unroll
        for (int r = 0; r < FISHER_CONV_PX; ++r) acc[r] += kj * fisher_conv_lds[r * GRAD_THREADS + (int)threadIdx.x + j];
    }
    double* __restrict__ out = J + ((size_t)w * D + k) * I.P + p0;
#pragma unroll
    for (int r = 0; r < FISHER_CONV_PX; ++r) {
        const int i = r * GRAD_THREADS + (int)threadIdx.x;
        if (i < nout) out[i] = acc[r];
    }
}

// part[w][chunk][j][k] (j <= k) = sum over the chunk's pixels of J_j[p] (w_p J_k[p]) for the rows of tile pair blockIdx.y.
// Lane = (lj, lk) of an 8 x 8 grid with a 4 x 4 block each; wave s takes pixels 16 s .. 16 s + 15 of every staged 64.
__global__ __launch_bounds__(GRAD_THREADS) void fisher_block_kernel(InstDev I, const double* __restrict__ lnprob, const double* __restrict__ J,
                                                                    int D, int nchunk, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) double lds[FISHER_PXT * FISHER_LDS_STRIDE];
    const int ch = blockIdx.x, w = blockIdx.z;
    if (!grad_row_valid(lnprob, w)) return;
    int tj = 0, tk = (int)blockIdx.y;                     // tile pair: (0,0) (0,1) .. (0,nt-1) (1,1) ..
    for (int nt = (D + FISHER_TILE - 1) / FISHER_TILE; tk >= nt - tj; tk -= nt - tj, ++tj) {}
    tk += tj;
    const int tid = threadIdx.x, s = tid >> 6, lane = tid & 63, lj = lane >> 3, lk = lane & 7;
    const double* __restrict__ Jw = J + (size_t)w * D * I.P;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    const int pbeg = ch * FISHER_CHUNK, pend = min(pbeg + FISHER_CHUNK, I.P);
    for (int q0 = pbeg; q0 < pend; q0 += FISHER_PXT) {    // (workgroup-uniform)
        // stage: column c < 32 = row tj * 32 + c, column 32 + c = w_p x row tk * 32 + c; zeros past D and past P
        const int px = tid & 63, p = q0 + px;
        const double wp = p < pend ? I.w[p] : 0.0;
        for (int c = tid >> 6; c < 2 * FISHER_TILE; c += GRAD_THREADS / 64) {
            const int rowi = c < FISHER_TILE ? tj * FISHER_TILE + c : tk * FISHER_TILE + c - FISHER_TILE;
            double v = 0.0;
            if (rowi < D && p < pend) v = Jw[(size_t)rowi * I.P + p];
            lds[px * FISHER_LDS_STRIDE + c] = c < FISHER_TILE ? v : wp * v;
        }
        __syncthreads();
#pragma unroll 4
        for (int pp = 0; pp < FISHER_PXT / 4; ++pp) {
            const double* __restrict__ at = lds + (s * (FISHER_PXT / 4) + pp) * FISHER_LDS_STRIDE;
            const double2 a01 = *reinterpret_cast<const double2*>(at + lj * 4), a23 = *reinterpret_cast<const double2*>(at + lj * 4 + 2);
            const double2 b01 = *reinterpret_cast<const double2*>(at + FISHER_TILE + lk * 4);
            const double2 b23 = *reinterpret_cast<const double2*>(at + FISHER_TILE + lk * 4 + 2);
            const double av[4] = {a01.x, a01.y, a23.x, a23.y}, bv[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_fma(av[a], bv[b], acc[a][b]);
        }
        __syncthreads();
    }
    // the four waves' slices, added in wave order by wave 0 (the staging buffer holds 4 x 64 x 16 doubles)
    static_assert(4 * 64 * 16 <= FISHER_PXT * FISHER_LDS_STRIDE, "reduction reuses the staging buffer");
    if (s > 0) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) lds[((s - 1) * 16 + a * 4 + b) * 64 + lane] = acc[a][b];
    }
    __syncthreads();
    if (s > 0) return;
    double* __restrict__ out = part + ((size_t)w * nchunk + ch) * D * D;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            double t = acc[a][b];
            for (int o = 0; o < 3; ++o) t += lds[(o * 16 + a * 4 + b) * 64 + lane];
            const int j = tj * FISHER_TILE + lj * 4 + a, k = tk * FISHER_TILE + lk * 4 + b;
            if (j <= k && k < D) out[(size_t)j * D + k] = t;
        }
}

// F[w][j][k] = F[w][k][j] = F[w][j][k] + sum over the chunks, in order.  One lane per (walker, j, k); lanes with j > k idle.
__global__ __launch_bounds__(GRAD_THREADS) void fisher_reduce_kernel(const double* __restrict__ lnprob, const double* __restrict__ part, int nchunk,
                                                                     int W, int D, double* __restrict__ F) {
    const long idx = (long)blockIdx.x * GRAD_THREADS + threadIdx.x;
    if (idx >= (long)W * D * D) return;
    const int w = (int)(idx / ((long)D * D)), jk = (int)(idx % ((long)D * D)), j = jk / D, k = jk % D;
    if (j > k || !grad_row_valid(lnprob, w)) return;
    double acc = 0.0;
    for (int c = 0; c < nchunk; ++c) acc += part[(((size_t)w * nchunk + c) * D + j) * D + k];
    double* __restrict__ Fw = F + (size_t)w * D * D;
    const double t = Fw[(size_t)j * D + k] + acc;
    Fw[(size_t)j * D + k] = t;
    Fw[(size_t)k * D + j] = t;
}

}  // namespace vp
