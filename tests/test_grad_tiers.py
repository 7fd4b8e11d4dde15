"""CPU side of the per-pixel derivative tests: the 40-digit grid tests/golden/wgrid/dwgrid.npz (its scales, its floors, its
regeneration) and the yardstick's rule grad_reference._hx_g against it.  The GPU side is tests/test_gpu_grad_tiers.py."""
import os
import sys

import numpy as np
from scipy.special import wofz

import grad_reference as gr

HERE = os.path.dirname(os.path.abspath(__file__))
GRID = os.path.join(HERE, "golden", "wgrid", "dwgrid.npz")
GRAD_RTOL = 1e-10            # tests/test_gpu_grad.py


def _generator():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_wgrid
    finally:
        sys.path.pop(0)
    return make_wgrid


def test_grid_scales_and_floors():
    """The scales in the file are the ones the generator defines, and the floors stay the exception: active on at most 5 % of
    the points and on none with |x| >= max(8, 2a) (a = 0 beyond the underflow of exp(-x^2) holds exact zeros: not counted)."""
    z = np.load(GRID)
    a, x, H, Hx, G = z["a"], z["x"], z["H"], z["Hx"], z["G"]
    assert np.all(a >= 0.0) and np.array_equal(x, -x[::-1])
    A, X = a[:, None], x[None, :]
    fG = 0.01 * np.abs(H) / (1.0 + X * X + A * A)
    fHx = 0.01 * np.abs(H) / (1.0 + np.hypot(X, A))
    assert np.array_equal(z["scale_G"], np.maximum(np.abs(G), fG)) and np.array_equal(z["scale_Hx"], np.maximum(np.abs(Hx), fHx))
    live = H != 0.0
    active = ((np.abs(G) < fG) | (np.abs(Hx) < fHx)) & live
    assert np.all(live[a > 0]) and active.sum() <= 0.05 * live.sum()
    assert not np.any(active & (np.abs(X) >= np.maximum(8.0, 2.0 * A)))
    # every boundary the device and the yardstick switch at has a point on it and one on either side
    for edge in (6.0, 8.0, 15.0, 36.0, 140.0, 600.0, 1e4):
        assert edge in x and np.nextafter(edge, 0.0) in x and -edge in x
    for edge in (8.0, 15.0, 36.0, 140.0, 600.0, 1e4):
        assert np.nextafter(edge, np.inf) in x
    for v in (29.9, 30.0):
        assert v in x
    for v in (0.15, 3.6, np.nextafter(7.0, 0.0), 7.0, 73.0, 0.1, np.nextafter(0.1, 1.0)):
        assert v in a


def test_grid_regenerates():
    """Recomputing a spread of points with the generator gives the stored float64 values.  The generator needs mpmath, and so
    does this test: without it the test fails (it does not skip), since nothing else ties the committed file to its recipe."""
    mk = _generator()
    z = np.load(GRID)
    assert np.array_equal(z["a"], mk.DW_A) and np.array_equal(z["x"], mk.DW_X)
    rng = np.random.default_rng(0)
    for i, j in zip(rng.integers(0, z["a"].size, 150), rng.integers(0, z["x"].size, 150)):
        v, d, g = mk.dw(z["x"][j], z["a"][i])
        assert (float(v.real), float(v.imag), float(d.real), float(g.real)) == (z["H"][i, j], z["L"][i, j], z["Hx"][i, j], z["G"][i, j])


def test_yardstick_rule_against_the_grid():
    """grad_reference._hx_g, fed scipy.special.wofz, against the grid, relative to the stored scales.  Where it sums the series
    (|z| >= 7 for a > 0.1, |z| >= 8 otherwise) it must stay within a tenth of what the GPU tests allow the device, GRAD_RTOL x
    scale: the yardstick may not use up the tolerance of what it judges.
    Below the switch it does not meet that tenth, and cannot with scipy's H (5e-14 |H| off near |x| = 6, which the rule
    multiplies by 2 x^4 / 3 in G).  Measured, of G's scale: 4.4e-11 for a <= 0.1 at |x| = 7.9 -- there the yardstick uses up 44 % of
    the tolerance of what it judges --, 4.2e-11 at a = 0.1+, |x| = 6.1, 1.2e-11 at a = 3.6, below 1.1e-11 elsewhere; 1.8e-12 of
    Hx's.  Nothing is loosened for it: the GPU tolerances stay, and what judges the device below the switch is the direct test
    against the grid (test_gpu_grad_tiers.test_voigt_dw_against_high_precision_grid), not this yardstick.  The assertion below
    the switch, 5e-11, only keeps the residue from growing unseen (a scipy whose wofz got worse near |x| = 6)."""
    z = np.load(GRID)
    a, x = z["a"], z["x"]
    A, X = np.meshgrid(a, x, indexing="ij")
    w = wofz(X + 1j * A)
    Hx, G = gr._hx_g(X, A, w.real, w.imag)
    r2 = X * X + A * A
    series = (r2 >= 64.0) | ((r2 >= gr.HXG_SERIES_Z ** 2) & (A > 0.1))
    floor = 1e-17 * (A == 0)             # wofz(x) and the series at a = 0, as in test_scipy_wofz_against_high_precision_grid
    eX, eG = np.abs(Hx - z["Hx"]), np.abs(G - z["G"])
    zz = np.sqrt(r2)
    for lo, hi in ((0, 5), (5, 6), (6, 7), (7, 8), (8, 15), (15, 30), (30, 100), (100, np.inf)):
        m = (zz >= lo) & (zz < hi)
        rX = np.where(eX <= floor, 0, eX / np.maximum(z["scale_Hx"], 1e-300))[m].max()
        rG = np.where(eG <= floor, 0, eG / np.maximum(z["scale_G"], 1e-300))[m].max()
        print("|z| in [%g, %g): worst |dHx| / scale = %.2e, |dG| / scale = %.2e" % (lo, hi, rX, rG))
    tol = np.where(series, 0.1 * GRAD_RTOL, 5e-11)
    assert np.all(eX <= tol * z["scale_Hx"] + floor)
    assert np.all(eG <= tol * z["scale_G"] + floor)


def test_rule_from_H_and_L_with_correctly_rounded_inputs():
    """What the fp64 rule  Hx = -2 (x H - a L),  G = H + a Ha + x Hx  gives when H and L are the correctly rounded values of the
    grid: the rounding of the rule alone.  It loses |z|^2 ulp in Hx and |z|^4 ulp in G, at every x once a is large.  Below
    |z| = 7, where the device (dw_generic, dw_fast's core) and the yardstick keep the rule, it stays within a tenth of GRAD_RTOL
    x scale; for a > 0.1 and |x| >= 100 -- most pixels of a line with b << 1 km/s -- it is beyond GRAD_RTOL x scale in G, by four
    orders at |x| = 1000: why both sum the series of w' and (z w)' there instead."""
    z = np.load(GRID)
    A, X = np.meshgrid(z["a"], z["x"], indexing="ij")
    H, L = z["H"], z["L"]
    Hx = -2 * (X * H - A * L)
    G = H + A * (2 * (X * L + A * H) - 2 / np.sqrt(np.pi)) + X * Hx
    rX = np.abs(Hx - z["Hx"]) / np.maximum(z["scale_Hx"], 1e-300)
    rG = np.abs(G - z["G"]) / np.maximum(z["scale_G"], 1e-300)
    zz = np.hypot(X, A)
    near = (zz < 7.0) & (H != 0)
    print("rule with exact H, L: |z| < 7: worst Hx %.2e, G %.2e of scale" % (rX[near].max(), rG[near].max()))
    assert rX[near].max() <= 0.1 * GRAD_RTOL and rG[near].max() <= 0.1 * GRAD_RTOL
    for lo, hi in ((30.0, 100.0), (100.0, 1000.0), (1000.0, np.inf)):
        m = (A > 0.1) & (np.abs(X) >= lo) & (np.abs(X) < hi)
        print("  a > 0.1, |x| in [%g, %g): worst Hx %.2e, G %.2e of scale" % (lo, hi, rX[m].max(), rG[m].max()))
    wings = (A > 0.1) & (np.abs(X) >= 100.0)
    assert rG[wings].max() > 1e4 * GRAD_RTOL and np.median(rG[wings]) > GRAD_RTOL


def _rule_from_H_and_L(x, a, H, L):
    Hx = -2 * (x * H - a * L)
    return Hx, H + a * (2 * (x * L + a * H) - 2 / np.sqrt(np.pi)) + x * Hx


def test_gradient_with_the_rule_from_H_and_L_outside_the_fast_domain():
    """The kernels' earlier rule inside the yardstick: Hx and G from H and L wherever a > 0.1, the yardstick's own rule elsewhere,
    on c0_mgii with the first component's b = 0.05, 0.002, 1e-4 (a = 0.15, 3.6, 73) and logN = 12, 14: the setup of
    test_gpu_fullsize.test_lines_outside_the_fast_domain and of the GPU gradient tests.  |dg_b| / S_b of that component against
    the yardstick proper, computed on the CPU: b = 0.05: 1.6e-14 / 3.3e-11, b = 0.002: 7.3e-7 / 8.0e-4, b = 1e-4: 7.7e-3 / 13 (logN =
    12 / 14).  So d lnL / d b was wrong by a multiple of its own scale for a state the value path supports; the assertions pin
    that the yardstick tells the two rules apart by far more than GRAD_RTOL where the GPU tests rely on it, that its S_b is
    positive and finite for these lines, and that at b = 0.05 (|z| < 7 at the pixels that carry S_b) both rules agree."""
    from oracle import voigt_oracle as vo
    z = np.load(os.path.join(HERE, "golden", "c0_mgii.npz"), allow_pickle=True)
    insts = vo.instruments_from_fixture(z)
    own = gr._hx_g

    def old_rule(x, a, H, L):
        Hx, G = own(x, a, H, L)
        Hx0, G0 = _rule_from_H_and_L(x, a, H, L)
        slow = np.broadcast_to(a > 0.1, np.shape(Hx))
        return np.where(slow, Hx0, Hx), np.where(slow, G0, G)

    worst = {}
    for b in (0.05, 0.002, 1e-4):
        for logN in (12.0, 14.0):
            th = z["theta_true"].copy()
            th[2], th[0] = b, logN
            _, g, S = gr.lnlike_grad(th, insts)
            gr._hx_g = old_rule
            try:
                _, g_old, S_old = gr.lnlike_grad(th, insts)
            finally:
                gr._hx_g = own
            assert np.all(np.isfinite(g)) and np.all(np.isfinite(S)) and np.all(S > 0)
            r = np.abs(g_old - g) / S
            worst[b, logN] = r
            print("b = %g, logN = %g: |dg| / S of the rule from H and L = %s" % (b, logN, np.array2string(r, precision=1)))
            assert np.all(r[[1, 3, 5]] <= GRAD_RTOL)              # the other component is a fast-domain line: untouched
    assert worst[0.05, 12.0][2] <= GRAD_RTOL and worst[0.05, 14.0][2] <= GRAD_RTOL
    for b in (0.002, 1e-4):
        for logN in (12.0, 14.0):
            assert worst[b, logN][2] > 1e3 * GRAD_RTOL
