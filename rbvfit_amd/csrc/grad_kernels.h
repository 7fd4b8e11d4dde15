// Reverse-mode gradient of lnprob (vp_lnprob_grad_batch*): d lnL / d theta in fp64, per walker row.
//
// With  tau_lp = T_l H(a_l, x_lp),  fl = exp(-sum_l tau_l),  m = LSF(fl),  lnL = -1/2 sum_p w_p (flux_p - m_p)^2 + const:
//     q_p = w_p (flux_p - m_p)                = d lnL / d m_p
//     u   = LSF^T q                             (transpose of the edge-replicated convolution: the clamped taps of the
//                                                outputs near either end pile onto pixel 0 and pixel P-1)
//     s_p = -u_p fl_p                         = d lnL / d tau_total,p
//     d lnL / d theta_k = sum_{l : idx(l) = k} sum_p s_p d tau_lp / d (logN | b | v)_l
//     d tau / d logN = ln(10) tau
//     d tau / d b    = -tau/b + T (H_a (-a/b) + H_x (-x/b)) = -(T/b) (H + a H_a + x H_x)
//     d tau / d v    = T H_x (freq_p / (c + v)) / b_f          (freq_p / b_f = x + freq0 / b_f)
//     H_x = -2 (x H - a L),  H_a = 2 (x L + a H) - 2/sqrt(pi),  w(x + i a) = H + i L   (voigt_w_device.h)
//
// Launches per instrument, all on one stream:  grad_prep_kernel (line records of the valid rows: prep_line_record, by call),
// grad_flux_kernel (fl: line_tau_wofz, by call -- the value path's own tier logic and its faithful x), grad_q_kernel, grad_s_kernel,
// grad_lines_kernel (one workgroup per (pixel chunk, line, walker): the three sums of a line over GRAD_CHUNK pixels, reduced over
// the workgroup in a fixed tree), grad_reduce_kernel (chunks in order, lines folded onto theta indices, instruments added
// in order).  No atomics anywhere: a row's bits depend on that row and the instrument tables alone.
//
// Rows whose lnprob is not finite (outside the box, NaN in theta, lnlike -inf / NaN) get a NaN gradient row; every kernel
// below leaves at once for such a row, so no model is evaluated for it.  None of the value kernels is touched.
#pragma once
#include "voigt_kernels.h"
#include "voigt_w_device.h"

namespace vp {

constexpr int GRAD_THREADS = 256;
constexpr int GRAD_PX = 8;                                // pixels per lane of grad_lines_kernel
constexpr int GRAD_CHUNK = GRAD_THREADS * GRAD_PX;        // pixels per workgroup of grad_lines_kernel
constexpr int GR_IB = 56, GR_RCV = 57;                    // free slots of a line record: 1/b, 1/(c + v)
constexpr double LN10 = 2.302585092994045684;

__device__ __forceinline__ bool grad_row_valid(const double* __restrict__ lnprob, int w) {
    return fabs(lnprob[w]) <= 1.79e308;                   // false for NaN and +-inf
}

__global__ __launch_bounds__(GRAD_THREADS) void grad_init_kernel(const double* __restrict__ lnprob, int W, int D, double* __restrict__ grad) {
    const long idx = (long)blockIdx.x * GRAD_THREADS + threadIdx.x;
    if (idx >= (long)W * D) return;
    grad[idx] = grad_row_valid(lnprob, (int)(idx / D)) ? 0.0 : __builtin_nan("");
}

// One lane per (walker, line) record.
__global__ __launch_bounds__(64) void grad_prep_kernel(const double* __restrict__ theta, const double* __restrict__ lnprob, int W, int D,
                                                       LinesDev T, double* __restrict__ rec) {
    const long idx = (long)blockIdx.x * 64 + threadIdx.x;
    if (idx >= (long)W * T.L) return;
    const int w = (int)(idx / T.L), l = (int)(idx % T.L);
    if (!grad_row_valid(lnprob, w)) return;
    const double* __restrict__ th = theta + (size_t)w * D;
    double* __restrict__ r = rec + (size_t)idx * LC_STRIDE;
    prep_line_record(th, T, l, r);
    r[GR_IB] = 1.0 / th[T.b_idx[l]];
    r[GR_RCV] = 1.0 / (C_KMS + th[T.v_idx[l]]);
}

// fl[w][p] = exp(-sum_l tau_lp)
__global__ __launch_bounds__(GRAD_THREADS) void grad_flux_kernel(InstDev I, const double* __restrict__ rec, const double* __restrict__ lnprob,
                                                                 double* __restrict__ fl) {
    const int w = blockIdx.y;
    if (!grad_row_valid(lnprob, w)) return;
    const int p = blockIdx.x * GRAD_THREADS + threadIdx.x;
    const int pc = min(p, I.P - 1);                       // (every lane stays active: the tiers are chosen by ballot)
    const PixelX xp{I.wave[pc], I.ginv[pc]};
    double tau = 0.0;
    for (int l = 0; l < I.L; ++l) tau += line_tau_wofz(xp, as_rec(rec + ((size_t)w * I.L + l) * LC_STRIDE));
    if (p < I.P) fl[(size_t)w * I.P + p] = exp(-tau);
}

// q[w][p] = w_p (flux_p - m_p),  m_p = sum_j kflip[j] fl[clamp(p - halo_lo + j)]
__global__ __launch_bounds__(GRAD_THREADS) void grad_q_kernel(InstDev I, const double* __restrict__ lnprob, const double* __restrict__ fl,
                                                              double* __restrict__ q) {
    const int w = blockIdx.y;
    if (!grad_row_valid(lnprob, w)) return;
    const int p = blockIdx.x * GRAD_THREADS + threadIdx.x;
    if (p >= I.P) return;
    const double* __restrict__ f = fl + (size_t)w * I.P;
    double m = 0.0;
    for (int j = 0; j < I.K; ++j) m += I.kflip[j] * f[min(max(p - I.halo_lo + j, 0), I.P - 1)];
    q[(size_t)w * I.P + p] = I.w[p] * (I.flux[p] - m);
}

// fl[w][p] <- s_p = -u_p fl_p,  u = LSF^T q
__global__ __launch_bounds__(GRAD_THREADS) void grad_s_kernel(InstDev I, const double* __restrict__ lnprob, const double* __restrict__ q,
                                                              double* __restrict__ fl) {
    const int w = blockIdx.y;
    if (!grad_row_valid(lnprob, w)) return;
    const int p = blockIdx.x * GRAD_THREADS + threadIdx.x;
    if (p >= I.P) return;
    const double* __restrict__ qw = q + (size_t)w * I.P;
    double u = 0.0;
    for (int j = 0; j < I.K; ++j) {
        const int pp = p + I.halo_lo - j;
        if (pp >= 0 && pp < I.P) u += I.kflip[j] * qw[pp];
    }
    if (p == 0) {              // output halo_lo - n sends its first n taps to pixel 0
        double cum = 0.0;
        for (int n = 1; n <= I.halo_lo; ++n) {
            cum += I.kflip[n - 1];
            const int pp = I.halo_lo - n;
            if (pp < I.P) u += qw[pp] * cum;
        }
    }
    if (p == I.P - 1) {        // output P-1 - (hi - n) sends its last n taps to pixel P-1
        const int hi = I.K - 1 - I.halo_lo;
        double cum = 0.0;
        for (int n = 1; n <= hi; ++n) {
            cum += I.kflip[I.K - n];
            const int pp = I.P - 1 - (hi - n);
            if (pp >= 0) u += qw[pp] * cum;
        }
    }
    const size_t at = (size_t)w * I.P + p;
    fl[at] = -u * fl[at];
}

// part[w][l][chunk][0..2] = sum over the chunk's pixels of s_p d tau_lp / d (logN, b, v)
__global__ __launch_bounds__(GRAD_THREADS) void grad_lines_kernel(InstDev I, const double* __restrict__ rec, const double* __restrict__ lnprob,
                                                                  const double* __restrict__ s, double* __restrict__ part, int nchunk) {
    const int ch = blockIdx.x, l = blockIdx.y, w = blockIdx.z;
    if (!grad_row_valid(lnprob, w)) return;
    rec_t r = as_rec(rec + ((size_t)w * I.L + l) * LC_STRIDE);
    const int mode = rec_int(r, LC_MODE, 0), nodd = rec_int(r, LC_MODE, 1);
    const double a = r[LC_Y], T = r[LC_T], ib = r[GR_IB], rcv = r[GR_RCV], B = r[LC_B];
    const double ea2 = ea2_small(a);
    const double* __restrict__ sw = s + (size_t)w * I.P;
    double accN = 0.0, accB = 0.0, accV = 0.0;
    for (int k = 0; k < GRAD_PX; ++k) {
        const int p0 = ch * GRAD_CHUNK + k * GRAD_THREADS;
        if (p0 >= I.P) break;                             // (workgroup-uniform)
        const int p = p0 + (int)threadIdx.x;
        const int pc = min(p, I.P - 1);
        const double x = faithful_x(I.wave[pc], I.ginv[pc], r);
        const DW h = dw_line(x, a, ea2, mode, nodd);
        const double sp = p < I.P ? sw[p] : 0.0;
        const double dN = LN10 * (T * h.H);
        const double dB = -(T * ib) * h.G;
        const double dV = T * h.Hx * ((x + B) * rcv);
        if (p < I.P) {                                    // (a lane past the end holds a copy of the last pixel: it adds nothing)
            accN += sp * dN;
            accB += sp * dB;
            accV += sp * dV;
        }
    }
    __shared__ double red[3][GRAD_THREADS / 64];
    const double sN = wave_sum(accN), sB = wave_sum(accB), sV = wave_sum(accV);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = sN;
        red[1][threadIdx.x >> 6] = sB;
        red[2][threadIdx.x >> 6] = sV;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double t = red[threadIdx.x][0];
        for (int k = 1; k < GRAD_THREADS / 64; ++k) t += red[threadIdx.x][k];
        part[(((size_t)w * I.L + l) * nchunk + ch) * 3 + threadIdx.x] = t;
    }
}

// grad[w][k] += sum over the lines tied to theta index k, chunks in order.  One lane per (walker, k).
__global__ __launch_bounds__(GRAD_THREADS) void grad_reduce_kernel(LinesDev T, const double* __restrict__ lnprob, const double* __restrict__ part,
                                                                   int nchunk, int W, int D, double* __restrict__ grad) {
    const long idx = (long)blockIdx.x * GRAD_THREADS + threadIdx.x;
    if (idx >= (long)W * D) return;
    const int w = (int)(idx / D), k = (int)(idx % D);
    if (!grad_row_valid(lnprob, w)) return;
    double acc = 0.0;
    for (int l = 0; l < T.L; ++l) {
        const double* __restrict__ pl = part + ((size_t)w * T.L + l) * nchunk * 3;
        if (T.N_idx[l] == k) for (int c = 0; c < nchunk; ++c) acc += pl[c * 3 + 0];
        if (T.b_idx[l] == k) for (int c = 0; c < nchunk; ++c) acc += pl[c * 3 + 1];
        if (T.v_idx[l] == k) for (int c = 0; c < nchunk; ++c) acc += pl[c * 3 + 2];
    }
    grad[idx] += acc;
}

// Test hook: w(x_j + i a_i), H and L (wave = 64 consecutive x_j of one a_i).  What dw_from_w consumes in the core (w_core_taylor)
// and outside the fast domain (w_generic); for 0 <= a <= 0.1 and |x| >= 8 the series are w_fast's own (voigt_dw_kernel shows
// what the gradient takes there).
__global__ __launch_bounds__(GRAD_THREADS) void voigt_w_kernel(const double* __restrict__ a, const double* __restrict__ x, int nx,
                                                               double* __restrict__ H, double* __restrict__ L) {
    const double ai = a[blockIdx.y];
    const int j = blockIdx.x * GRAD_THREADS + threadIdx.x;
    const double xj = x[min(j, nx - 1)];
    const bool fast = ai >= 0.0 && ai <= 0.1;             // (uniform: one a per workgroup)
    const W2 h = fast ? w_fast(xj, ai, ea2_small(ai), core_terms(ai)) : w_generic(xj, ai);
    if (j < nx) {
        H[(size_t)blockIdx.y * nx + j] = h.H;
        L[(size_t)blockIdx.y * nx + j] = h.L;
    }
}

// Test hook: H, Hx = Re w', G = Re (z w)' at (x_j, a_i) through dw_line, the function grad_lines_kernel calls, with the mode and
// the term count a line record of that a would carry (wave = 64 consecutive x_j of one a_i).
__global__ __launch_bounds__(GRAD_THREADS) void voigt_dw_kernel(const double* __restrict__ a, const double* __restrict__ x, int nx,
                                                                double* __restrict__ H, double* __restrict__ Hx, double* __restrict__ G) {
    const double ai = a[blockIdx.y];
    const int j = blockIdx.x * GRAD_THREADS + threadIdx.x;
    const double xj = x[min(j, nx - 1)];                  // (every lane stays active: the tiers are chosen by ballot)
    const DW h = dw_line(xj, ai, ea2_small(ai), dw_mode(ai), core_terms(ai));
    if (j < nx) {
        const size_t at = (size_t)blockIdx.y * nx + j;
        H[at] = h.H;
        Hx[at] = h.Hx;
        G[at] = h.G;
    }
}

}  // namespace vp
