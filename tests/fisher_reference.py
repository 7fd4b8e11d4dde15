"""CPU yardstick for the model Jacobian and the Fisher matrix (a helper, not a test): NumPy on top of ``grad_reference``.

``jacobian(theta, inst, convolved=True) -> (J (D, P), A (D, P))`` and ``fisher(theta, instruments) -> (F (D, D), FA (D, D))``.

    tau_l = A_l H(a_l, x_l),  fl = exp(-sum_l tau_l)
    g_k   = -fl sum_{(l, kind) : idx(l, kind) = k} d tau_l / d (logN | b | v)_l        (tied parameters fold here)
    J_k   = LSF(g_k) = d model_flux / d theta_k,     F = sum_inst J W J^T,  W = diag(inv_sigma2)

The forward part repeats ``grad_reference.lnlike_grad``'s operations in its order; ``_hx_g`` gives H_x and G, and
``voigt_oracle.lsf_convolve`` is the LSF.  ``A`` is ``J`` with every (line, pixel) term replaced by its absolute value before
the convolution, which then runs with |taps|; ``FA_jk = sum_p w_p A_j[p] A_k[p]``.  A and FA are the scales the Jacobian and
Fisher tolerances are relative to, as S_k is for the gradient (the terms of a tied parameter, and the taps of a kernel
with negative lobes, cancel).
"""
import numpy as np
from scipy.special import wofz

from oracle import voigt_oracle as vo
import grad_reference as gr

C_KMS = gr.C_KMS


def line_terms(theta, inst):
    """(fl (P,), [(dt (L, P), idx (L,)) for logN, b, v]): the unconvolved flux and d tau_lp / d (logN | b | v)_l of every line."""
    theta = np.asarray(theta, dtype=np.float64)
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
    Hx, G = gr._hx_g(x, a, H, L)
    dt_dN = np.log(10) * tau
    dt_db = -(A / b) * G
    dt_dv = A * Hx * (freq / (C_KMS + v)) / b_f
    fl = np.exp(-np.sum(tau, axis=0))
    return fl, ((dt_dN, d.N_indices), (dt_db, d.b_indices), (dt_dv, d.v_indices))


def _abs_taps(data):
    """|taps| as the LSF applies them (the astropy branch divides by the sum of the taps first), for LSF_SCIPY_NEAREST."""
    if data.lsf_mode == vo.LSF_NONE or data.taps is None or len(data.taps) == 0:
        return None
    k = np.asarray(data.taps, dtype=np.float64)
    if data.lsf_mode == vo.LSF_ASTROPY_EXTEND:
        k = k / k.sum()
    return np.abs(k)


def jacobian(theta, inst, convolved=True):
    theta = np.asarray(theta, dtype=np.float64)
    D, P = theta.size, inst.wave.size
    fl, kinds = line_terms(theta, inst)
    g, a = np.zeros((D, P)), np.zeros((D, P))
    for dt, idx in kinds:
        np.add.at(g, idx, dt)                      # lines in line order
        np.add.at(a, idx, np.abs(dt))
    g *= -fl[None, :]
    a *= fl[None, :]
    if not convolved:
        return g, a
    d = inst.data
    ka = _abs_taps(d)
    J = np.array([vo.lsf_convolve(row, d.taps, d.lsf_mode) for row in g])
    A = a if ka is None else np.array([vo.lsf_convolve(row, ka, vo.LSF_SCIPY_NEAREST) for row in a])
    return J, A


def fisher(theta, instruments):
    theta = np.asarray(theta, dtype=np.float64)
    D = theta.size
    F, FA = np.zeros((D, D)), np.zeros((D, D))
    for inst in instruments:
        J, A = jacobian(theta, inst)
        w = np.asarray(inst.inv_sigma2, dtype=np.float64)
        F += (J * w[None, :]) @ J.T
        FA += (A * w[None, :]) @ A.T
    return F, FA


def scaled_condition(F):
    """cond of F / sqrt(diag x diag) (inf when a diagonal entry is not positive)."""
    d = np.diag(F)
    if not np.all(d > 0):
        return np.inf
    s = np.sqrt(d)
    lam = np.linalg.eigvalsh(F / np.outer(s, s))
    return np.inf if lam[0] <= 0 else float(lam[-1] / lam[0])
