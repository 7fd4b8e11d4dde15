// Complex Faddeeva function w(x + i a) = H + i L for the gradient path (grad_kernels.h).  fp64 throughout.
//
// The value kernels need H = Re w alone (voigt_device.h).  The derivatives of the optical depth need L = Im w beside it:
//     dH/dx = -2 (x H - a L),      dH/da = 2 (x L + a H) - 2/sqrt(pi)        (from w' = -2 z w + 2i/sqrt(pi)).
// The tiers are those of voigt_device.h, each carried to the imaginary part; the functions there are left as they are
// and none of the value kernels calls anything in this file.
//
//   |x| >= 8, 0 <= a <= 0.1 : asymptotic series  w ~ (i / (sqrt(pi) z)) sum_m (2m-1)!! / (2 z^2)^m  in complex arithmetic.
//                             With s = 1/z^2 every product that enters Im of the sum has one sign, so H (of order a/x^2
//                             beside L of order 1/x) keeps its relative accuracy.  M in {2,3,4,6,9,14} terms by |x|.
//   |x| <  8, 0 <= a <= 0.1 : the Taylor series of voigt_device.h in the damping direction; the same v_n recurrence gives both parts:
//                                 H =  e^{a^2-x^2} cos(2ax) - a v_1 + a^3 v_3 - ...
//                                 L = -e^{a^2-x^2} sin(2ax) + v_0 - a^2 v_2 + a^4 v_4 - ...
//   a > 0.1                 : Gaussian-sum form of ACM TOMS Alg. 916 (Zaghloul & Ali 2011), both parts, for |x| < 6 and a < 7;
//                             the Gautschi / Poppe-Wijers continued fraction elsewhere.  a < 0: reflection w(z) = 2 e^{-z^2} - w(-z).
#pragma once
#include "voigt_device.h"

namespace vp {

struct W2 { double H, L; };

// Asymptotic series, |x| >= 8 and 0 <= a <= 0.1 (M = 14 there; fewer terms farther out, see w_fast).
template <int M>
__device__ __forceinline__ W2 w_wing(double x, double a) {
    const double inv = fast_rcp(x * x + a * a);
    const double zr = x * inv, zi = -a * inv;                  // 1/z
    const double sr = zr * zr - zi * zi, si = 2.0 * zr * zi;   // 1/z^2
    double c[M];
    c[0] = 1.0;
#pragma unroll
    for (int m = 1; m < M; ++m) c[m] = c[m - 1] * (0.5 * (double)(2 * m - 1));
    double pr = c[M - 1], pi = 0.0;
#pragma unroll
    for (int m = M - 2; m >= 0; --m) {
        const double t = pr * sr - pi * si + c[m];
        pi = pr * si + pi * sr;
        pr = t;
    }
    const double qr = zr * pr - zi * pi, qi = zr * pi + zi * pr;
    return W2{-INV_SQRT_PI * qi, INV_SQRT_PI * qr};
}

// Taylor tier: |x| < 8, 0 <= a <= 0.1.  `nodd` = core_terms(a), `ea2` = exp(a^2).
__device__ __forceinline__ W2 w_core_taylor(double x, double a, double ea2, int nodd) {
    const double ax = fabs(x);
    const int i = min((int)(ax * 2.0), DAW_NI - 1);
    const double t = __builtin_fma(ax, 4.0, -(double)(2 * i + 1));
    const double* __restrict__ cf = &g_dawson[i][0][0];
    double F = cf[DAW_DEG], G = cf[DAW_DEG + 1 + DAW_DEG];
#pragma unroll
    for (int k = DAW_DEG - 1; k >= 0; --k) {
        F = __builtin_fma(F, t, cf[k]);
        G = __builtin_fma(G, t, cf[DAW_DEG + 1 + k]);
    }
    G = (i >= DAW_GLO) ? G : __builtin_fma(-2.0 * ax, F, 1.0);
    const double c = 1.1283791670955125739;          // 2/sqrt(pi)
    double vp = c * F, vc = c * G;                    // v_0, v_1
    const double E = exp_neg(ax * ax) * ea2;
    const double a2 = a * a;
    double apow = -a;                                 // odd powers with the alternating sign folded in
    double epow = 1.0;                                // even powers, likewise
    double accH = apow * vc, accL = vp;
    constexpr double R[12] = {-1.0, -2.0 / 3, -0.5, -0.4, -2.0 / 6, -2.0 / 7, -0.25, -2.0 / 9, -0.2, -2.0 / 11,
                              -2.0 / 12, -2.0 / 13};
#pragma unroll
    for (int k = 1; k < 7; ++k) {
        if (k < nodd) {                               // wave-uniform
            const double v1 = R[2 * k - 2] * __builtin_fma(ax, vc, vp);     // v_{2k}
            const double v2 = R[2 * k - 1] * __builtin_fma(ax, v1, vc);     // v_{2k+1}
            vp = v1; vc = v2;
            apow = -apow * a2;
            epow = -epow * a2;
            accH = __builtin_fma(apow, vc, accH);
            accL = __builtin_fma(epow, vp, accL);
        }
    }
    {   // one more even term: the odd series ends at a^(2 nodd - 1), the even one would end a power lower
        const double v1 = (-2.0 / (double)(2 * nodd)) * __builtin_fma(ax, vc, vp);
        accL = __builtin_fma(-epow * a2, v1, accL);
    }
    const double th = a * ax;
    const double sn2 = 2.0 * th * sinc_small(2.0 * th);
    W2 w;
    w.H = __builtin_fma(E, cos_small(2.0 * th), accH);
    const double L = __builtin_fma(-E, sn2, accL);
    w.L = x < 0.0 ? -L : L;                           // L is odd in x
    return w;
}

// Continued fraction (large |z|, any a >= 0), both parts; x >= 0.
__device__ inline W2 w_cf(double ax, double y) {
    if (ax + y > 1e7) {   // w ~ i / (sqrt(pi) z), scaled against overflow
        if (ax > y) { const double yax = y / ax, d = INV_SQRT_PI / (ax + yax * y); return W2{d * yax, d}; }
        const double xya = ax / y, d = INV_SQRT_PI / (xya * ax + y);
        return W2{d, d * xya};
    }
    double nu = floor(3.9 + 11.398 / (0.08254 * ax + 0.1421 * y + 0.2023));
    double wr = ax, wi = y;
    for (nu = 0.5 * (nu - 1.0); nu > 0.4; nu -= 0.5) {
        const double denom = nu / (wr * wr + wi * wi);
        wr = ax - wr * denom;
        wi = y + wi * denom;
    }
    const double d = INV_SQRT_PI / (wr * wr + wi * wi);
    return W2{d * wi, d * wr};
}

// Alg. 916, both parts: 0 <= x < 6, 0.1 < y < 7.  Table-free (a rare path: unphysical damping).
__device__ inline W2 w_alg916(double ax, double y) {
    const double E = exp(-ax * ax);
    double s1 = 0.0, s23 = 0.0, s54 = 0.0;
    for (int n = 1; n <= NCORE; ++n) {
        const double hn = ALG916_H * n;
        const double tb = exp(-hn * hn) / (hn * hn + y * y);
        const double ep = exp(2.0 * hn * ax), em = exp(-2.0 * hn * ax);
        s1 += tb;
        s23 += tb * (ep + em);
        s54 += (hn * tb) * (ep - em);
    }
    const double t = ax * y;
    const double sn = sin(t), sn2 = sin(2.0 * t), cs2 = cos(2.0 * t);
    const double coef1 = erfcx(y) - ALG916_C * y * s1;
    const double coef2 = ALG916_C * ax;
    W2 w;
    w.H = E * (coef1 * cs2 + coef2 * sn * sinc_safe(t, sn) + 0.5 * ALG916_C * y * s23);
    w.L = E * (coef2 * sinc_safe(2.0 * t, sn2) - coef1 * sn2 + 0.5 * ALG916_C * s54);
    return w;
}

// Any (x, a): per-lane branches, slow, rare in the kernels (a > 0.1 or a < 0).
__device__ inline W2 w_generic(double x, double a) {
    if (!(fabs(a) <= 1.79e308) || !(fabs(x) <= 1.79e308)) return W2{__builtin_nan(""), __builtin_nan("")};
    const double ax = fabs(x), y = fabs(a);
    W2 w = (y >= 7.0 || ax >= 6.0) ? w_cf(ax, y) : w_alg916(ax, y);
    if (a < 0.0) {        // w(x - iy) = 2 e^{y^2 - x^2} (cos 2xy + i sin 2xy) - conj(w(x + iy))
        const double g = 2.0 * exp(y * y - ax * ax);
        w.H = g * cos(2.0 * ax * y) - w.H;
        w.L = g * sin(2.0 * ax * y) + w.L;
    }
    if (x < 0.0) w.L = -w.L;
    return w;
}

// exp(a^2) for a <= 0.1: seven Taylor terms, remainder a^14/5040 < 2e-18 (the gradient kernels form it themselves
// and do not take the records' LC_EA2, whose five terms leave 8e-13 at a = 0.1)
__device__ __forceinline__ double ea2_small(double a) {
    const double a2 = a * a;
    return 1.0 + a2 * (1.0 + a2 * (0.5 + a2 * (1.0 / 6 + a2 * (1.0 / 24 + a2 * (1.0 / 120 + a2 * (1.0 / 720))))));
}

// What the derivatives of tau need of w at one (x, a):  H,  Hx = dH/dx = Re w',  G = H + a dH/da + x dH/dx = Re (z w)'.
//     d tau / d logN = ln(10) T H,    d tau / d v = T Hx (x + freq0/b_f) / (c + v),    d tau / d b = -(T / b) G
// (a and x are both proportional to 1/b).  From H and L,  Hx = -2 (x H - a L)  and  G = H + a Ha + x Hx  with
// Ha = 2 (x L + a H) - 2/sqrt(pi): fine near the core, but in the wings both are small differences of large terms
// (Hx ~ a/x^3 from two terms ~ a/x;  G ~ a/x^4 from terms ~ a/x^2: a Lorentzian wing does not depend on b) and lose
// x^2 ulp.  There the series of w' and (z w)' are summed directly.
struct DW { double H, Hx, G; };

__device__ __forceinline__ DW dw_from_w(double x, double a, W2 w) {
    const double Hx = -2.0 * (x * w.H - a * w.L);
    const double Ha = 2.0 * (x * w.L + a * w.H) - 2.0 * INV_SQRT_PI;
    return DW{w.H, Hx, w.H + a * Ha + x * Hx};
}

// |x| >= 8, 0 <= a <= 0.1.  With s = 1/z^2, c_m = (2m-1)!!/2^m, P0 = sum c_m s^m, P2 = sum_{m>=1} 2m c_m s^m:
//     w = (i/sqrt(pi)) (1/z) P0,    w' = -(i/sqrt(pi)) s (P0 + P2),    (z w)' = -(i/sqrt(pi)) (1/z) P2
template <int M>
__device__ __forceinline__ DW dw_wing(double x, double a) {
    const double inv = fast_rcp(x * x + a * a);
    const double zr = x * inv, zi = -a * inv;                  // 1/z
    const double sr = zr * zr - zi * zi, si = 2.0 * zr * zi;   // 1/z^2
    double c[M];
    c[0] = 1.0;
#pragma unroll
    for (int m = 1; m < M; ++m) c[m] = c[m - 1] * (0.5 * (double)(2 * m - 1));
    double pr = c[M - 1], pi = 0.0, gr = (double)(2 * (M - 1)) * c[M - 1], gi = 0.0;
#pragma unroll
    for (int m = M - 2; m >= 0; --m) {
        const double t = pr * sr - pi * si + c[m];
        pi = pr * si + pi * sr;
        pr = t;
        const double u = gr * sr - gi * si + (double)(2 * m) * c[m];
        gi = gr * si + gi * sr;
        gr = u;
    }
    const double qi = zr * pi + zi * pr;                       // Im (P0 / z)
    const double hi = zr * gi + zi * gr;                       // Im (P2 / z)
    const double tr = pr + gr, ti = pi + gi;                   // P0 + P2
    const double di = sr * ti + si * tr;                       // Im (s (P0 + P2))
    return DW{-INV_SQRT_PI * qi, INV_SQRT_PI * di, INV_SQRT_PI * hi};
}

__device__ __forceinline__ DW dw_fast(double x, double a, double ea2, int nodd) {
    const double xa = fabs(x);
    const bool nanx = !(xa <= 1.79e308);
    if (__ballot(xa < X_CORE || nanx) == 0ull) {
        if (__ballot(xa < 10000.0) == 0ull) return dw_wing<3>(x, a);
        if (__ballot(xa < 600.0) == 0ull) return dw_wing<4>(x, a);
        if (__ballot(xa < 140.0) == 0ull) return dw_wing<5>(x, a);
        if (__ballot(xa < 36.0) == 0ull) return dw_wing<7>(x, a);
        if (__ballot(xa < 15.0) == 0ull) return dw_wing<10>(x, a);
        return dw_wing<NWING + 1>(x, a);
    }
    DW d = dw_from_w(x, a, w_core_taylor(x, a, ea2, nodd));
    if (__ballot(xa >= X_CORE) != 0ull) {
        const DW dd = dw_wing<NWING + 1>(x, a);
        if (xa >= X_CORE) d = dd;
    }
    if (nanx) { d.H = __builtin_nan(""); d.Hx = d.H; d.G = d.H; }
    return d;
}

// Outside the fast domain (a > 0.1, a < 0): per-lane branches, slow, rare.  H and L of w_generic are good to 1e-13 |H|, but Hx and G
// formed from them lose |z|^2 and |z|^4 ulp at every x once a is large (a line with a > 0.1 has b << 1 km/s: nearly all of its
// pixels lie at |x| >> 100, where G from H and L is noise).  So from |z| = 7 on the series of w' and (z w)' are summed directly,
// as in the fast domain: the series in 1/z^2 does not care how large a is; 24 terms leave 4e-14 of G at |z| = 7.2 and 1e-13 at 7
// (against the 40-digit grid, tests/golden/wgrid/dwgrid.npz).  Below |z| = 7 (a < 7 there) H and L come from the Gaussian sum
// also for 6 <= |x| < 7, where its 26 terms still hold (3e-15 |H|): the continued fraction w_generic takes from |x| = 6 is 1e-13 |H|
// off at small a, which the rule multiplies by 2 x^4 / 3 in G.
constexpr int NWING_GENERIC = 24;
constexpr double Z2_GENERIC_SERIES = 49.0;

__device__ inline DW dw_generic(double x, double a) {
    const double r2 = x * x + a * a;
    if (a > 0.1 && r2 >= Z2_GENERIC_SERIES && r2 <= 1.79e308) return dw_wing<NWING_GENERIC>(x, a);
    if (a > 0.1 && r2 < Z2_GENERIC_SERIES) {
        W2 w = w_alg916(fabs(x), a);
        if (x < 0.0) w.L = -w.L;
        return dw_from_w(x, a, w);
    }
    return dw_from_w(x, a, w_generic(x, a));              // a < 0 (reflection), NaN, |z|^2 beyond the range
}

// LC_MODE[0] of a line's record as fill_record sets it from a (finite T): 0: 0 <= a <= 0.1, 1: 0.1 < a < 7, 2: a >= 7 or a < 0,
// 3: not finite.  For the test hook, which has no record.
__device__ __forceinline__ int dw_mode(double a) {
    if (!(fabs(a) <= 1.79e308)) return 3;
    if (!(a >= 0.0) || !(a < 7.0)) return 2;
    return a > 0.1 ? 1 : 0;
}

// The derivatives of w at one pixel of one line: what grad_lines_kernel accumulates and what the test hook vp_voigt_dw shows.
// `mode`, `nodd`: LC_MODE of the line's record (wave-uniform); mode 0: every lane of the wave must be active (dw_fast).
__device__ __forceinline__ DW dw_line(double x, double a, double ea2, int mode, int nodd) {
    return (mode == 0) ? dw_fast(x, a, ea2, nodd) : dw_generic(x, a);
}

// Fast domain (0 <= a <= 0.1), tier by wavefront like line_tau_wofz: every lane of the wave must be active.  Only the hook
// vp_voigt_w calls it: its |x| >= 8 series (w_wing) are the hook's own, the gradient kernels take dw_wing there.
__device__ __forceinline__ W2 w_fast(double x, double a, double ea2, int nodd) {
    const double xa = fabs(x);
    const bool nanx = !(xa <= 1.79e308);
    if (__ballot(xa < X_CORE || nanx) == 0ull) {
        if (__ballot(xa < 10000.0) == 0ull) return w_wing<2>(x, a);
        if (__ballot(xa < 600.0) == 0ull) return w_wing<3>(x, a);
        if (__ballot(xa < 140.0) == 0ull) return w_wing<4>(x, a);
        if (__ballot(xa < 36.0) == 0ull) return w_wing<6>(x, a);
        if (__ballot(xa < 15.0) == 0ull) return w_wing<9>(x, a);
        return w_wing<NWING>(x, a);
    }
    W2 w = w_core_taylor(x, a, ea2, nodd);
    if (__ballot(xa >= X_CORE) != 0ull) {
        const W2 ww = w_wing<NWING>(x, a);
        if (xa >= X_CORE) w = ww;
    }
    if (nanx) { w.H = __builtin_nan(""); w.L = w.H; }
    return w;
}

}  // namespace vp
