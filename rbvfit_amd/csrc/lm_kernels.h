// Batched Levenberg-Marquardt fit (vp_lm_run, vp_lm_solve): fp64, per walker row, no atomics.
//
// lnprob(theta + d) ~ lnprob + g^T d - 1/2 d^T F d  with F the Fisher matrix (fisher_kernels.h) and g the gradient (grad_kernels.h).
// One iteration of a row:
//     held_k = (theta_k on a bound and g_k points outward) | !(F_kk > 0) | F_kk (ub_k - lb_k)^2 < freeze_tol      (d_k = 0)
//     free set, s = sqrt(diag F):  C = F / (s s^T),  gh = g / s,  (C + lambda I) y = gh,  d = y / s                  (Marquardt's scaling)
//     theta_trial = clip(theta + d, lb, ub),   pred = gh^T y - 1/2 y^T C y = 1/2 (gh^T y + lambda y^T y)
//     accept if lnprob(theta_trial) is finite and > lnprob; lambda by Nielsen's rule; status 0 running, 1 converged, 2 start not
//     evaluable, 3 stalled (lambda > lambda_max)
//
// lm_step_kernel: one workgroup per row, one lane per free index (D <= LM_MAX_D).  The scaled matrix is a packed lower triangle in
// LDS; left-looking Cholesky, column by column (lane i forms L_ij from the finished columns k < j, k ascending), then the two
// triangular solves column by column.  Every element is written by one lane in an order fixed by (i, j) alone, and the three sums
// behind pred and |y|_inf are one lane's loops: a row's bits depend on that row alone, whatever the workgroup's size.  A pivot
// that is not positive ends the row's solve with ok = 0 (the driver raises lambda: not an error).
// lm_mask_kernel hands the Fisher / gradient launches a lnprob vector that is finite only for the rows they are to evaluate (those
// kernels leave at once for the others); lm_keep_kernel copies the evaluated rows' blocks into the rows' persistent F and g.
#pragma once
#include "grad_kernels.h"

namespace vp {

constexpr int LM_MAX_D = 96;                              // LDS at D = 96: 40.5 KB (the packed triangle's 96 x 97 / 2 doubles, five D-vectors, pos)
constexpr int LM_THREADS = 256;                           // lm_accept_kernel / lm_init_kernel: one workgroup, rows strided

// doubles: A (D (D + 1) / 2) | s (D) | rhs (D) | z (D) | gh (D) | Ld (D);  ints: pos (D) | n, failed
__host__ __device__ inline size_t lm_step_lds_bytes(int D) {
    return ((size_t)D * (D + 1) / 2 + 5 * (size_t)D) * sizeof(double) + ((size_t)D + 2) * sizeof(int);
}

struct LmStep {
    const double *F, *g, *theta, *lb, *ub, *lambda;       // (W, D, D) | (W, D) | (W, D) | (D) | (D) | (W)
    const int* status;                                    // (W) rows with status != 0 are left alone (NULL: every row is solved)
    double freeze_tol;
    double *trial, *pred, *ynorm;                         // (W, D) | (W) | (W)
    int *held, *ok;                                       // (W, D) or NULL | (W)
};

__global__ __launch_bounds__(LM_THREADS) void lm_step_kernel(LmStep a, int D) {
    extern __shared__ __attribute__((aligned(16))) double lm_lds[];
    const int w = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    const double* __restrict__ th = a.theta + (size_t)w * D;
    double* __restrict__ trial = a.trial + (size_t)w * D;
    if (a.status && a.status[w] != 0) {                   // (workgroup-uniform)
        for (int k = tid; k < D; k += T) trial[k] = th[k];
        if (tid == 0) { a.pred[w] = 0.0; a.ynorm[w] = 0.0; a.ok[w] = 1; }
        return;
    }
    double* A = lm_lds;
    double* s = A + (size_t)D * (D + 1) / 2;
    double* rhs = s + D;
    double* z = rhs + D;
    double* gh = z + D;
    double* Ld = gh + D;
    int* pos = reinterpret_cast<int*>(Ld + D);
    int* nfo = pos + D;                                   // [0] free indices, [1] the solve failed
    const double* __restrict__ Fw = a.F + (size_t)w * D * D;
    const double* __restrict__ gw = a.g + (size_t)w * D;
    const double lam = a.lambda[w];
    for (int k = tid; k < D; k += T) {
        const double dk = Fw[(size_t)k * D + k], gk = gw[k], t = th[k], lo = a.lb[k], hi = a.ub[k], width = hi - lo;
        const bool hk = (t == lo && gk < 0.0) || (t == hi && gk > 0.0) || !(dk > 0.0) || dk * width * width < a.freeze_tol;
        s[k] = hk ? 1.0 : sqrt(dk);
        pos[k] = hk ? -1 : 0;
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int k = 0; k < D; ++k) if (pos[k] == 0) pos[k] = n++;
        nfo[0] = n;
        nfo[1] = 0;
    }
    __syncthreads();
    const int n = nfo[0];
    for (int e = tid; e < D * D; e += T) {                // (coalesced over the row-major block; the lower triangle is kept)
        const int r = e / D, q = e - r * D;
        if (q > r || pos[r] < 0 || pos[q] < 0) continue;
        const int i = pos[r], j = pos[q];
        double v = Fw[e] / (s[r] * s[q]);
        if (i == j) v += lam;
        A[i * (i + 1) / 2 + j] = v;
    }
    for (int k = tid; k < D; k += T)
        if (pos[k] >= 0) rhs[pos[k]] = gh[pos[k]] = gw[k] / s[k];
    __syncthreads();
    // left-looking Cholesky: lane i owns row i (the host launches T >= D lanes)
    const int i = tid, ii = i * (i + 1) / 2;
    bool failed = false;
    for (int j = 0; j < n; ++j) {
        const int jj = j * (j + 1) / 2;
        if (i >= j && i < n) {
            double acc = A[ii + j];
            for (int k = 0; k < j; ++k) acc = __builtin_fma(-A[ii + k], A[jj + k], acc);
            A[ii + j] = acc;
        }
        __syncthreads();
        const double piv = A[jj + j];
        if (!(piv > 0.0) || !(piv <= 1.79e308)) { failed = true; break; }      // (workgroup-uniform: every lane reads the same word)
        const double dj = sqrt(piv);
        if (i == j) Ld[j] = dj;
        if (i > j && i < n) A[ii + j] = A[ii + j] / dj;
        __syncthreads();
    }
    if (!failed) {
        for (int j = 0; j < n; ++j) {                     // L z = gh, column by column
            const double zj = rhs[j] / Ld[j];
            if (i == j) z[j] = zj;
            if (i > j && i < n) rhs[i] = __builtin_fma(-A[ii + j], zj, rhs[i]);
            __syncthreads();
        }
        for (int j = n - 1; j >= 0; --j) {                // L^T y = z; y lands in rhs
            const double yj = z[j] / Ld[j];
            if (i == j) rhs[j] = yj;
            if (i < j) z[i] = __builtin_fma(-A[j * (j + 1) / 2 + i], yj, z[i]);
            __syncthreads();
        }
    }
    if (tid == 0) {
        double gy = 0.0, yy = 0.0, ymax = 0.0;
        bool good = !failed;
        for (int k = 0; good && k < n; ++k) {
            const double y = rhs[k];
            good = fabs(y) <= 1.79e308;
            gy = __builtin_fma(gh[k], y, gy);
            yy = __builtin_fma(y, y, yy);
            ymax = fmax(ymax, fabs(y));
        }
        nfo[1] = good ? 0 : 1;
        a.pred[w] = good ? 0.5 * (gy + lam * yy) : 0.0;
        a.ynorm[w] = good ? ymax : 0.0;
        a.ok[w] = good ? 1 : 0;
    }
    __syncthreads();
    const bool good = nfo[1] == 0;
    for (int k = tid; k < D; k += T) {
        const double t = th[k];
        const bool hk = pos[k] < 0;
        double v = t;
        if (good && !hk) v = fmin(fmax(t + rhs[pos[k]] / s[k], a.lb[k]), a.ub[k]);
        trial[k] = v;
        if (a.held) a.held[(size_t)w * D + k] = hk ? 1 : 0;
    }
}

// The persistent state of the rows of a vp_lm_run call.
struct LmState {
    double *theta, *lp, *lam, *nu;                        // (W, D) | (W) | (W) | (W)
    int *status, *niter, *nacc, *stale;                   // (W) each; stale: F and g are not those of theta
    int* running;                                         // one word: rows with status 0 after the last lm_init / lm_accept launch
};

// the workgroup's count of running rows (one workgroup holds every row)
__device__ __forceinline__ void lm_store_running(int mine, int* running) {
    __shared__ int cnt[LM_THREADS];
    cnt[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int k = 0; k < LM_THREADS; ++k) n += cnt[k];
        *running = n;
    }
}

__global__ __launch_bounds__(LM_THREADS) void lm_init_kernel(int W, LmState S, double lambda0) {
    int mine = 0;
    for (int w = threadIdx.x; w < W; w += LM_THREADS) {
        const bool ok = grad_row_valid(S.lp, w);
        S.status[w] = ok ? 0 : 2;
        S.lam[w] = lambda0;
        S.nu[w] = 2.0;
        S.niter[w] = 0;
        S.nacc[w] = 0;
        S.stale[w] = 1;
        mine += ok ? 1 : 0;
    }
    lm_store_running(mine, S.running);
}

// out[w] = lnprob of the rows whose F and g are to be evaluated (stale, evaluable and -- need_running -- still running), NaN for the others
__global__ __launch_bounds__(LM_THREADS) void lm_mask_kernel(int W, LmState S, int need_running, double* __restrict__ out) {
    const int w = blockIdx.x * LM_THREADS + threadIdx.x;
    if (w >= W) return;
    const int st = S.status[w];
    const bool take = S.stale[w] != 0 && st != 2 && (!need_running || st == 0);
    out[w] = take ? S.lp[w] : __builtin_nan("");
}

// F[w], g[w] <- Ft[w], gt[w] for the rows the masked launches evaluated (mask[w] finite); their stale flag is cleared.  gt may be NULL.
__global__ __launch_bounds__(LM_THREADS) void lm_keep_kernel(int W, int D, const double* __restrict__ mask, const double* __restrict__ Ft,
                                                             const double* __restrict__ gt, double* __restrict__ F, double* __restrict__ g,
                                                             int* __restrict__ stale) {
    const int per = D * D + D;
    const long idx = (long)blockIdx.x * LM_THREADS + threadIdx.x;
    if (idx >= (long)W * per) return;
    const int w = (int)(idx / per), e = (int)(idx - (long)w * per);
    if (!grad_row_valid(mask, w)) return;
    if (e < D * D) F[(size_t)w * D * D + e] = Ft[(size_t)w * D * D + e];
    else if (gt) g[(size_t)w * D + (e - D * D)] = gt[(size_t)w * D + (e - D * D)];
    if (e == 0) stale[w] = 0;
}

// One lane per row: the trial's lnprob decides; lambda, status and the counters follow.
__global__ __launch_bounds__(LM_THREADS) void lm_accept_kernel(int W, int D, LmState S, const double* __restrict__ trial,
                                                               const double* __restrict__ lp_trial, const double* __restrict__ pred,
                                                               const double* __restrict__ ynorm, const int* __restrict__ ok, double ftol,
                                                               double xtol, double lambda_max) {
    int mine = 0;
    for (int w = threadIdx.x; w < W; w += LM_THREADS) {
        if (S.status[w] != 0) continue;
        int st = 0;
        double lam = S.lam[w], nu = S.nu[w];
        const double lp = S.lp[w], lt = lp_trial[w];
        S.niter[w] += 1;
        bool accepted = false;
        if (ok[w]) {
            if (fabs(lt) <= 1.79e308 && lt > lp) {
                accepted = true;
                const double gain = lt - lp, rho = gain / pred[w], u = 2.0 * rho - 1.0;
                if (gain <= ftol * fmax(1.0, fabs(lp))) st = 1;
                lam *= fmax(1.0 / 3.0, 1.0 - u * u * u);
                nu = 2.0;
                for (int k = 0; k < D; ++k) S.theta[(size_t)w * D + k] = trial[(size_t)w * D + k];
                S.lp[w] = lt;
                S.nacc[w] += 1;
                S.stale[w] = 1;
            }
            if (ynorm[w] <= xtol) st = 1;
        }
        if (!accepted) { lam *= nu; nu *= 2.0; }
        if (st == 0 && lam > lambda_max) st = 3;
        S.lam[w] = lam;
        S.nu[w] = nu;
        S.status[w] = st;
        mine += st == 0 ? 1 : 0;
    }
    lm_store_running(mine, S.running);
}

}  // namespace vp
