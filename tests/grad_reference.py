"""CPU yardstick for the analytic gradient (a helper, not a test): NumPy / scipy.special.wofz on top of the oracle's objects.

``lnlike_grad(theta, instruments) -> (lnlike, grad (D,), S (D,))``.  The forward part repeats ``oracle.voigt_oracle``'s
operations in its order (so lnlike agrees with ``voigt_oracle.lnlike`` to rounding); the derivatives are calculus:

    tau = A H(a, x),  A = N f constant;   fl = exp(-sum_l tau_l);   m = LSF(fl);   q = inv_sigma2 (flux - m);   u = LSF^T q;   s = -u fl
    d tau / d logN = ln(10) tau
    d tau / d b    = -tau/b + A (H_a (-a/b) + H_x (-x/b)) = -(A/b) (H + a H_a + x H_x)
    d tau / d v    = A H_x (freq / (c + v)) / b_f
    H_x = -2 (x H - a L),  H_a = 2 (x L + a H) - 2/sqrt(pi),   w(x + i a) = H + i L

``S_k`` is the same sum as ``grad_k`` with every (line, pixel) term replaced by its absolute value: the scale the gradient
tolerances are relative to (the terms cancel heavily).
"""
import numpy as np
from scipy.special import wofz

from oracle import voigt_oracle as vo

C_KMS = 299792.458


def lsf_transpose(q, taps, lsf_mode):
    """u = M^T q for the matrix M of ``voigt_oracle.lsf_convolve`` (out[p] = sum_j k[j] fl[clamp(p + c - j)]): the clamped
    taps of the outputs near either end pile onto pixel 0 and pixel P-1."""
    q = np.asarray(q, dtype=np.float64)
    if lsf_mode == vo.LSF_NONE or taps is None or len(taps) == 0:
        return q.copy()
    k = np.asarray(taps, dtype=np.float64)
    if lsf_mode == vo.LSF_ASTROPY_EXTEND:
        k = k / k.sum()
    P, K = q.size, k.size
    c = K // 2
    u = np.zeros(P)
    for j in range(K):
        np.add.at(u, np.clip(np.arange(P) + c - j, 0, P - 1), k[j] * q)
    return u


HXG_SERIES_Z = 7.0          # |z| from which _hx_g sums the asymptotic series
HXG_SERIES_TERMS = 24


def _hx_g(x, a, H, L):
    """H_x and G = H + a H_a + x H_x (so that d tau / d b = -(A / b) G: a and x are both proportional to 1/b).
    From H and L both are small differences of large terms once |z| is large (H_x ~ a/x^3 from two terms ~ a/x, G ~ a/x^4 from
    terms ~ a/x^2: a Lorentzian wing does not depend on b; for large a the same at every x) and lose |z|^2 and |z|^4 ulp -- more
    than the tolerance of the GPU tests for a line that lies outside the spectrum, or one with a > 0.1.  For |z| >= 7 the
    asymptotic series of w' and (z w)' are summed instead (c_m = (2m-1)!!/2^m, s = 1/z^2):
        w' = -(i/sqrt(pi)) s sum (2m+1) c_m s^m,      (z w)' = -(i/sqrt(pi)) (1/z) sum 2m c_m s^m,
    24 terms (the terms shrink up to m = |z|^2 = 49; the first one left out is 1e-13 of the sum at |z| = 7), in real arithmetic
    on (Re, Im) pairs: complex division would round Im s ~ a/x^3 against |s| ~ 1/x^2 and lose x/a ulp for a narrow line.
    For a <= 0.1 the series start at |z| = 8: the Gaussian exp(-x^2) (1 - 2 x^2), which no term of the series holds, is 5e-20 at
    |x| = 7 beside G = 8e-4 a there, 6e-11 of it for a = 1e-6; at |x| = 8 it is 3e-17 of it.
    Against the 40-digit grid (tests/test_grad_tiers.py) this is within 2e-13 of the scales of tests/golden/make_wgrid.py from
    |z| = 7 on; below, scipy's H decides (worst: 4.2e-11 of G's scale at a = 0.1, |x| = 6.1, where wofz is 5e-14 |H| off)."""
    x, a, H, L = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (x, a, H, L)))
    Hx = -2 * (x * H - a * L)
    Ha = 2 * (x * L + a * H) - 2 / np.sqrt(np.pi)
    G = H + a * Ha + x * Hx
    far = (x * x + a * a >= 64.0) | ((x * x + a * a >= HXG_SERIES_Z ** 2) & (a > 0.1))
    if np.any(far):
        xf, af = np.where(far, x, HXG_SERIES_Z), np.where(far, a, 0.0)
        inv = 1.0 / (xf * xf + af * af)
        zr, zi = xf * inv, -af * inv                              # 1/z
        sr, si = zr * zr - zi * zi, 2.0 * zr * zi                 # 1/z^2
        c = np.cumprod(np.concatenate([[1.0], 0.5 * (2 * np.arange(1, HXG_SERIES_TERMS) - 1)]))
        p1r, p1i, p2r, p2i = (np.zeros_like(sr) for _ in range(4))
        for m in range(HXG_SERIES_TERMS - 1, -1, -1):
            p1r, p1i = p1r * sr - p1i * si + (2 * m + 1) * c[m], p1r * si + p1i * sr
            p2r, p2i = p2r * sr - p2i * si + (2 * m) * c[m], p2r * si + p2i * sr
        k = 1.0 / np.sqrt(np.pi)                                  # Re (-i k (u + i v)) = k v
        Hx = np.where(far, k * (sr * p1i + si * p1r), Hx)
        G = np.where(far, k * (zr * p2i + zi * p2r), G)
    return Hx, G


def lnlike_grad(theta, instruments):
    theta = np.asarray(theta, dtype=np.float64)
    D = theta.size
    g, S, total = np.zeros(D), np.zeros(D), 0.0
    for inst in instruments:
        d = inst.data
        lam0 = d.atomic_lambda0[:, None]
        gam = d.atomic_gamma[:, None]
        f = d.atomic_f[:, None]
        N = (10 ** theta[d.N_indices])[:, None]
        b = theta[d.b_indices][:, None]
        v = theta[d.v_indices]
        z_total = d.z_factors * (1 + v / C_KMS) - 1
        wave_rest = inst.wave[None, :] / (1 + z_total[:, None])
        v = v[:, None]
        b_f = b / lam0 * 1e13
        freq0 = 2.99792458e18 / lam0
        freq = 2.99792458e18 / wave_rest
        constant = 4.48898479507e3 / (freq0 * b)
        a = gam / (4 * np.pi * b_f)
        x = (freq - freq0) / b_f
        w = wofz(x + 1j * a)
        H, L = w.real, w.imag
        A = N * f * constant
        tau = A * H
        Hx, G = _hx_g(x, a, H, L)
        dt_dN = np.log(10) * tau
        dt_db = -(A / b) * G
        dt_dv = A * Hx * (freq / (C_KMS + v)) / b_f
        fl = np.exp(-np.sum(tau, axis=0))
        m = vo.lsf_convolve(fl, d.taps, d.lsf_mode)
        r = inst.flux - m
        total += -0.5 * np.sum(r ** 2 * inst.inv_sigma2 - inst.log_inv_sigma2)
        u = lsf_transpose(inst.inv_sigma2 * r, d.taps, d.lsf_mode)
        s = -u * fl
        for dt, idx in ((dt_dN, d.N_indices), (dt_db, d.b_indices), (dt_dv, d.v_indices)):
            terms = dt * s[None, :]
            np.add.at(g, idx, terms.sum(axis=1))
            np.add.at(S, idx, np.abs(terms).sum(axis=1))
    return total, g, S
