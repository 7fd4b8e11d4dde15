"""The CPU side of the analytic gradient: the yardstick (tests/grad_reference.py) against the oracle, against high-precision
w(z), against the dense matrix of the LSF and against finite differences of the oracle; and the C ABI of the new entries."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.special import wofz

from oracle import voigt_oracle as vo
import grad_reference as gr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
NEW_SYMBOLS = ["vp_lnprob_grad_batch", "vp_lnprob_grad_batch_device", "vp_voigt_w", "vp_voigt_dw"]
FD_FIXTURES = ["c0_mgii", "c0_mgii_nolsf", "c3_mini", "tiny_7px", "dla_lya"]


def _load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=True)
    return z, vo.instruments_from_fixture(z)


def _finite_rows(z, insts, n):
    rows = [t for t in np.atleast_2d(z["thetas"]) if np.isfinite(vo.lnprob(t, z["lb"], z["ub"], insts))]
    assert len(rows) >= n
    return rows[:n]


@pytest.mark.parametrize("name", FD_FIXTURES + ["c2_mini", "c4_mini", "real_cos"])
def test_helper_lnlike_is_the_oracles(name):
    z, insts = _load(name)
    for t in _finite_rows(z, insts, 2):
        ref = vo.lnlike(t, insts)
        got = gr.lnlike_grad(t, insts)[0]
        assert abs(got - ref) <= 1e-12 * abs(ref)


def test_scipy_wofz_against_high_precision_grid():
    """scipy.special.wofz is the yardstick's ingredient for L = Im w.  Against tests/golden/wgrid/wgrid.npz (mpmath, 40 digits)
    its worst deviation is 5.2e-14 |H| in H (a = 0.1+, |x| = 6) and 1.9e-14 max(|L|, |H|) in L; relative to |L| alone
    1.2e-13 (a = 7).  Rows with a = 0 get the absolute floor 1e-17 in H (wofz returns exp(-x^2) there)."""
    z = np.load(os.path.join(GOLD, "wgrid", "wgrid.npz"))
    a, x, H, L = z["a"], z["x"], z["H"], z["L"]
    w = wofz(x[None, :] + 1j * a[:, None])
    dH, dL = np.abs(w.real - H), np.abs(w.imag - L)
    assert np.all(dH <= 1e-12 * np.abs(H) + 1e-17 * (a[:, None] == 0))
    assert np.all(dL <= 1e-12 * np.maximum(np.abs(L), np.abs(H)))


@pytest.mark.parametrize("mode", [vo.LSF_SCIPY_NEAREST, vo.LSF_ASTROPY_EXTEND])
@pytest.mark.parametrize("P", [1, 3, 7, 40, 64])
def test_lsf_transpose_is_the_matrix_transpose(mode, P):
    k = np.load(os.path.join(GOLD, "conv_semantics.npz"))["kernel"]
    assert not np.allclose(k, k[::-1])                    # asymmetric: an unflipped kernel would show
    M = np.stack([vo.lsf_convolve(e, k, mode) for e in np.eye(P)], axis=1)      # column i = LSF(e_i)
    q = np.random.default_rng(P).normal(size=P)
    ref = M.T @ q
    got = gr.lsf_transpose(q, k, mode)
    assert np.max(np.abs(got - ref)) <= 1e-14 * np.sum(np.abs(ref))


def _richardson(t, insts):
    def central(h):
        out = np.zeros(t.size)
        for k in range(t.size):
            e = np.zeros(t.size)
            e[k] = h
            out[k] = (vo.lnlike(t + e, insts) - vo.lnlike(t - e, insts)) / (2 * h)
        return out
    return (4 * central(5e-5) - central(1e-4)) / 3


@pytest.mark.parametrize("name", FD_FIXTURES)
def test_formulas_against_finite_differences_of_the_oracle(name):
    z, insts = _load(name)
    for t in _finite_rows(z, insts, 3):
        _, g, S = gr.lnlike_grad(t, insts)
        fd = _richardson(t, insts)
        ratio = np.abs(g - fd) / S
        print(name, "worst |g - g_fd| / S = %.2e" % ratio.max())
        assert np.all(np.abs(g - fd) <= 1e-5 * S)


def test_new_symbols_declared_and_exported():
    import __graft_entry__ as ge
    ge.build()
    with open(os.path.join(ROOT, "include", "rbvfit_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(vp_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", ge.LIB], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    from rbvfit_amd import _lib
    for s in NEW_SYMBOLS:
        assert s in declared and s in exported and s in _lib.SIGNATURES, s
