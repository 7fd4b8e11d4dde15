"""GPU tests of what the analytic gradient takes per pixel, tier by tier, and of the configurations its parity tests leave out.

1. vp_voigt_dw (the device function grad_lines_kernel calls, dw_line) against tests/golden/wgrid/dwgrid.npz: H, Hx = Re w' and
   G = Re (z w)' at 40 digits, on and beside every boundary of the series of the fast domain, of w_generic and of the series
   that take over outside the fast domain, laid over the waves in three ways so that every series runs.  Bounds: H within
   1e-12 |H|; Hx and G within GRAD_RTOL times the scales stored in the file (|Hx|, |G| themselves away from their sign changes:
   tests/golden/make_wgrid.py).  The bound is derived, not measured: if every term of sum_p s_p dtau_p is within 1e-10 of its
   own size, the sum is within 1e-10 S_k, which is what the gradient tests promise.
2. lnprob_grad with a line outside the fast domain (a = 0.15, 3.6, 73 on MgII), alone, beside quiet rows, and off the spectrum.
3. lnprob_grad on the seeded random configurations of test_gpu_fuzz and on its 72- and 132-line cases.

Measured worst ratios, before and after the series outside the fast domain: profiles/grad_notes.md."""
import os

import numpy as np
import pytest

from conftest import load_golden
from helpers import engine_from_fixture
from oracle import voigt_oracle as vo
import grad_reference as gr
from test_gpu_grad import GRAD_RTOL, _check_rows, _same_bits

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
A_CLASSES = [("0 <= a <= 0.1", lambda a: a <= 0.1), ("0.1 < a < 7", lambda a: (a > 0.1) & (a < 7.0)), ("a >= 7", lambda a: a >= 7.0)]


# ---- 1. the per-pixel derivatives ----------------------------------------------------------------------------------------
# the |x| bands of dw_fast and what it runs in each when a whole wave lies inside one (chosen by ballot over the wave)
X_BANDS = [(0.0, 6.0, "core"), (6.0, 8.0, "core"), (8.0, 15.0, "dw_wing<15>"), (15.0, 36.0, "dw_wing<10>"), (36.0, 140.0, "dw_wing<7>"),
           (140.0, 600.0, "dw_wing<5>"), (600.0, 1e4, "dw_wing<4>"), (1e4, np.inf, "dw_wing<3>")]


def _dw_on_device(eng, a, x, order):
    """The hook on the whole grid, in the column order of x.  `sorted` and `mixed`: one call, 117 x = two waves per a, each of
    which holds core pixels (|x| < 8) in either order, so for 0 <= a <= 0.1 every pixel beyond 8 goes through the fall-through
    to dw_wing<NWING + 1> and the per-lane blend of core and wing: these two orders never run a shorter series.  `banded`: one
    call per |x| band with that band's x alone (fewer than 64: one wave per a, whose idle lanes hold a copy of the band's last
    x), so the ballots of dw_fast pick the band's own series: dw_wing<10>, <7>, <5>, <4>, <3> run here and only here."""
    if order == "banded":
        out = [np.empty((a.size, x.size)) for _ in range(3)]
        for lo, hi, _ in X_BANDS:
            m = np.nonzero((np.abs(x) >= lo) & (np.abs(x) < hi))[0]
            assert 0 < m.size <= 64
            for o, g in zip(out, eng.voigt_dw(a, x[m])):
                o[:, m] = g
        return out
    idx = np.argsort(x) if order == "sorted" else np.random.default_rng(5).permutation(x.size)
    out = [np.empty((a.size, x.size)) for _ in range(3)]
    for o, g in zip(out, eng.voigt_dw(a, x[idx])):
        o[:, idx] = g
    return out


@pytest.mark.parametrize("order", ["sorted", "mixed", "banded"])
def test_voigt_dw_against_high_precision_grid(order):
    """Three layouts of the same grid over the waves (see _dw_on_device): together they run every series of dw_fast, the
    fall-through and the blend.  Outside the fast domain the choice is per lane and the layout does not matter.
    The a = 0 rows get the absolute floor 1e-17 of the w(z) test where the device sums the asymptotic series, |x| >= 8: the series
    holds no exp(-x^2) < 2e-28, all that is left of H, Hx and G at a = 0.  Below 8 they are held to the relative bounds."""
    import rbvfit_amd
    z = np.load(os.path.join(HERE, "golden", "wgrid", "dwgrid.npz"))
    a, x = z["a"], z["x"]
    assert np.all(a >= 0.0)
    with rbvfit_amd.Engine(0) as eng:
        gH, gHx, gG = _dw_on_device(eng, a, x, order)
    floor = 1e-17 * ((a[:, None] == 0) & (np.abs(x)[None, :] >= 8.0))
    err, bound = {}, {}
    for name, got, scale, rtol in (("H", gH, np.abs(z["H"]), 1e-12), ("Hx", gHx, z["scale_Hx"], GRAD_RTOL), ("G", gG, z["scale_G"], GRAD_RTOL)):
        err[name] = np.abs(got - z[name])
        bound[name] = rtol * scale
    ratio = {k: np.where(err[k] <= floor, 0.0, err[k] / np.maximum(bound[k], 1e-300)) for k in err}
    for label, sel in A_CLASSES:
        for lo, hi, tier in X_BANDS:
            m = sel(a)[:, None] & ((np.abs(x) >= lo) & (np.abs(x) < hi))[None, :]
            ran = "dw_generic" if label != A_CLASSES[0][0] else tier if order == "banded" or hi <= 8.0 else "dw_wing<15> by lane"
            print("%-6s %-14s |x| in [%g, %g) %-19s worst error / bound  H %.2e  Hx %.2e  G %.2e"
                  % (order, label, lo, hi, ran + ":", ratio["H"][m].max(), ratio["Hx"][m].max(), ratio["G"][m].max()))
    for k in ("H", "Hx", "G"):
        bad = np.argwhere(~(err[k] <= bound[k] + floor))
        assert bad.size == 0, "%s: %d points beyond the bound, worst error / bound = %.3e; first: a = %g, x = %g" % (
            k, len(bad), np.nanmax(ratio[k]), a[bad[0][0]], x[bad[0][1]])


# ---- 2. lines outside the fast domain ------------------------------------------------------------------------------------
def _slow_line_case(b_value, logN, v=None):
    """The setup of test_gpu_fullsize.test_lines_outside_the_fast_domain: c0_mgii with the first component's b tiny."""
    z = load_golden("c0_mgii")
    th = z["theta_true"].copy()
    th[2], th[0] = b_value, logN
    lb, ub = z["lb"].copy(), z["ub"].copy()
    lb[2] = 0.0
    if v is not None:
        th[4] = v
        ub[4] = max(ub[4], v + 100.0)
    return z, th, lb, ub


@pytest.mark.parametrize("logN", [12.0, 14.0])
@pytest.mark.parametrize("b_value", [0.05, 0.002, 1e-4])
def test_gradient_with_a_line_outside_the_fast_domain(b_value, logN):
    """b = 0.05 -> a ~ 0.15; 0.002 -> a ~ 3.6; 1e-4 -> a ~ 73.  Alone, and interleaved with theta_true rows: a row's bits must
    not depend on its neighbours, and the quiet rows keep the bits they have in a batch of their own."""
    z, th, lb, ub = _slow_line_case(b_value, logN)
    insts = vo.instruments_from_fixture(z)
    label = "b = %g, logN = %g" % (b_value, logN)
    with engine_from_fixture(z) as eng:
        eng.set_bounds(lb, ub)
        _check_rows(eng, th, lb, ub, insts, label + ", alone")
        lp1, g1 = eng.lnprob_grad(th)
        quiet = np.tile(z["theta_true"], (9, 1))
        lpq, gq = eng.lnprob_grad(quiet)
        mixed = quiet.copy()
        mixed[::3] = th
        _check_rows(eng, mixed, lb, ub, insts, label + ", interleaved")
        lpm, gm = eng.lnprob_grad(mixed)
        assert np.all(np.isfinite(lp1)) and np.all(np.isfinite(g1))
        for w in range(len(mixed)):
            if w % 3 == 0:
                assert _same_bits(gm[w], g1[0]) and _same_bits(lpm[w:w + 1], lp1), "%s: row %d differs from the row alone" % (label, w)
            else:
                assert _same_bits(gm[w], gq[w]) and _same_bits(lpm[w:w + 1], lpq[w:w + 1]), "%s: quiet row %d moved" % (label, w)


@pytest.mark.parametrize("b_value", [0.002, 1e-4])
def test_gradient_with_such_a_line_off_the_spectrum(b_value):
    """The first component moved by v = +2100 km/s: both of its transitions lie beyond the red end of the spectrum, every pixel
    is a far-wing pixel of them (|x| > 100 asserted below), and S_b of that component consists of such terms alone."""
    z, th, lb, ub = _slow_line_case(b_value, 14.0, v=2100.0)
    insts = vo.instruments_from_fixture(z)
    lam = z["G__lambda0"][z["G__b_idx"] == 2] * z["G__zfac"][z["G__b_idx"] == 2] * (1 + th[4] / gr.C_KMS)
    wave = z["G__wave"]
    assert np.all(lam > wave.max())
    x_min = gr.C_KMS * (lam.min() - wave.max()) / lam.min() / b_value          # Doppler widths from the nearest pixel
    assert x_min > 100.0
    with engine_from_fixture(z) as eng:
        eng.set_bounds(lb, ub)
        _check_rows(eng, np.vstack([th, z["theta_true"], th]), lb, ub, insts, "b = %g off the spectrum (|x| >= %.3g)" % (b_value, x_min))


# ---- 3. seeded random configurations -------------------------------------------------------------------------------------
def _oracle_side(model, wave, err, thetas, rng):
    data = model.compile().data
    od = vo.OracleModelData(data.atomic_lambda0, data.atomic_gamma, data.atomic_f, data.z_factors, data.N_indices,
                            data.b_indices, data.v_indices, data.taps if data.taps is not None else np.zeros(0),
                            data.lsf_mode, data.voigt_method)
    flux = vo.model_flux(od, thetas[0], wave) + rng.normal(0, 1, wave.size) * err
    return data, vo.OracleInstrument.from_error(od, wave, flux, err), flux


@pytest.mark.parametrize("seed", range(36))
def test_gradient_of_random_configuration(seed):
    """The 36 configurations of test_gpu_fuzz.test_random_configuration (descending and jittered grids, the asymmetric
    tabulated kernel on the astropy branch, clusters, damped components, 2-38 lines), all six rows of each.  Seeds 4, 13, 22
    and 31 are voigt_method='fast': refused with VP_EINVAL, asserted.  Every row of the other 32 has a finite lnprob."""
    import rbvfit_amd
    from rbvfit_amd._lib import RbvfitAmdError, VP_EINVAL
    from test_gpu_fuzz import _random_case
    model, wave, err, thetas, lb, ub, rng = _random_case(seed)
    data, inst, flux = _oracle_side(model, wave, err, thetas, rng)
    with rbvfit_amd.Engine(0) as e:
        e.set_bounds(lb, ub)
        e.add_instrument(wave, flux, inst.inv_sigma2, inst.log_inv_sigma2, **data.engine_kwargs())
        if seed % 9 == 4:
            with pytest.raises(RbvfitAmdError, match="voigt_method 'fast'") as ei:
                e.lnprob_grad(thetas)
            assert ei.value.code == VP_EINVAL
            return
        assert np.all(np.isfinite(e.lnprob(thetas))), "seed %d: every row has a finite lnprob" % seed
        _check_rows(e, thetas, lb, ub, [inst], "seed %d (%d lines, %d px)" % (seed, data.n_lines, wave.size))


@pytest.mark.parametrize("n_sys,comps", [(2, 9), (3, 11)])
def test_gradient_with_more_than_64_and_128_lines(n_sys, comps):
    """The 72- and 132-line configurations of test_gpu_fuzz.test_more_than_64_and_128_lines (2 and 3 mask words of the value
    path, whose lnprob the gradient call returns), through the yardstick; theta and noise drawn per case."""
    import rbvfit_amd
    from rbvfit_amd.model import FitConfiguration, VoigtModel
    rng = np.random.default_rng(99 + n_sys)
    cfg = FitConfiguration()
    for s in range(n_sys):
        cfg.add_system(0.30 + 0.004 * s, "FeII", [2600.1729, 2586.650, 2382.765, 2344.214], comps)
    model = VoigtModel(cfg, FWHM="4.0")
    C = cfg.total_components
    wave = np.linspace(3030.0, 3420.0, 7000)
    theta = np.concatenate([rng.uniform(12.5, 14.5, C), rng.uniform(5, 40, C), rng.uniform(-200, 200, C)])
    lb = np.concatenate([np.full(C, 10.0), np.full(C, 1.0), np.full(C, -400.0)])
    ub = np.concatenate([np.full(C, 18.0), np.full(C, 150.0), np.full(C, 400.0)])
    thetas = np.clip(theta + 0.05 * rng.standard_normal((4, 3 * C)), lb + 1e-9, ub - 1e-9)
    data, inst, flux = _oracle_side(model, wave, np.full(wave.size, 0.05), thetas, rng)
    assert data.n_lines == n_sys * 4 * comps
    with rbvfit_amd.Engine(0) as e:
        e.set_bounds(lb, ub)
        e.add_instrument(wave, flux, inst.inv_sigma2, inst.log_inv_sigma2, **data.engine_kwargs())
        assert np.all(np.isfinite(e.lnprob(thetas)))
        _check_rows(e, thetas, lb, ub, [inst], "%d lines" % data.n_lines)
