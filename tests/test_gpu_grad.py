"""GPU tests of the analytic gradient (vp_lnprob_grad_batch*, vp_voigt_w) against the CPU yardstick tests/grad_reference.py.

Every gradient tolerance is relative to S_k, the sum of the absolute values of the terms of component k (the terms cancel
heavily: S_k / |g_k| reaches 900 on the committed fixtures).  Measured worst ratios: profiles/grad_notes.md."""
import os

import numpy as np
import pytest

from conftest import load_golden, LNPROB_RTOL
from helpers import engine_from_fixture
from oracle import voigt_oracle as vo
import grad_reference as gr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GRAD_RTOL = 1e-10            # x S_k: the project's lnprob tolerance carried over to the same kind of sum
PARITY = ["c0_mgii", "c0_mgii_nolsf", "c0_mgii_strong", "c2_mini", "c2_window", "c3_mini", "c4_mini", "dla_lya", "tiny_7px",
          "one_px", "ragged_1000", "real_cos"]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _check_rows(eng, thetas, lb, ub, insts, label):
    """lnprob + gradient of every row against Engine.lnprob and the yardstick; returns the worst |dg| / S."""
    thetas = np.atleast_2d(thetas)
    lp, g = eng.lnprob_grad(thetas)
    ref_lp = eng.lnprob(thetas)
    assert lp.shape == (len(thetas),) and g.shape == thetas.shape
    assert np.array_equal(np.isneginf(lp), np.isneginf(ref_lp)) and np.array_equal(np.isnan(lp), np.isnan(ref_lp)), label
    fin = np.isfinite(ref_lp)
    assert np.all(np.abs(lp[fin] - ref_lp[fin]) <= LNPROB_RTOL * np.abs(ref_lp[fin])), label
    assert np.all(np.isnan(g[~fin])), label + ": rows without a finite lnprob must get a NaN gradient row"
    worst = 0.0
    for w in np.nonzero(fin)[0]:
        _, gh, S = gr.lnlike_grad(thetas[w], insts)
        ratio = np.abs(g[w] - gh) / S
        worst = max(worst, float(np.max(ratio)))
        assert np.all(np.abs(g[w] - gh) <= GRAD_RTOL * S), "%s row %d: worst |dg|/S = %.3e" % (label, w, np.max(ratio))
    print("%s: %d finite rows of %d, worst |g - g_ref| / S = %.3e" % (label, fin.sum(), len(thetas), worst))
    return worst


# ---- 1. w(z) -------------------------------------------------------------------------------------------------------------
W_BANDS = [0.0, 8.0, 15.0, 36.0, 140.0, 600.0, 1e4, np.inf]          # w_fast: core, then w_wing<14>, <9>, <6>, <4>, <3>, <2>


@pytest.mark.parametrize("order", ["sorted", "mixed", "banded"])
def test_voigt_w_against_high_precision_grid(order):
    """`sorted`, `mixed`: one call, 95 x = two waves per a, each with core pixels in it: every |x| >= 8 of the fast domain goes
    through the per-lane blend with w_wing<NWING>.  `banded`: one call per |x| band of w_fast (one wave per a, idle lanes hold
    the band's last x), so that the ballots pick the band's own shorter series."""
    import rbvfit_amd
    z = np.load(os.path.join(HERE, "golden", "wgrid", "wgrid.npz"))
    a, x, H, L = z["a"], z["x"], z["H"], z["L"]
    gH, gL = np.empty_like(H), np.empty_like(L)
    with rbvfit_amd.Engine(0) as eng:
        if order == "banded":
            for lo, hi in zip(W_BANDS[:-1], W_BANDS[1:]):
                m = np.nonzero((np.abs(x) >= lo) & (np.abs(x) < hi))[0]
                assert 0 < m.size <= 64
                gH[:, m], gL[:, m] = eng.voigt_w(a, x[m])
        else:
            idx = np.argsort(x) if order == "sorted" else np.random.default_rng(5).permutation(x.size)
            gH[:, idx], gL[:, idx] = eng.voigt_w(a, x[idx])
    floor = 1e-17 * (a[:, None] == 0)
    eH = np.abs(gH - H) / np.maximum(np.abs(H), 1e-300)
    eL = np.abs(gL - L) / np.maximum(np.maximum(np.abs(L), np.abs(H)), 1e-300)
    print("%s: worst |dH|/|H| = %.3e, worst |dL|/max(|L|,|H|) = %.3e" % (order, np.max(np.where(np.abs(gH - H) <= floor, 0, eH)), eL.max()))
    assert np.all(np.abs(gH - H) <= 1e-12 * np.abs(H) + floor)
    assert np.all(np.abs(gL - L) <= 1e-12 * np.maximum(np.abs(L), np.abs(H)))


# ---- 2. parity on the fixtures (also: tied parameters, several instruments: c3_mini, c4_mini) ------------------------------
@pytest.mark.parametrize("name", PARITY)
def test_gradient_parity(name):
    z = load_golden(name)
    insts = vo.instruments_from_fixture(z)
    eng = engine_from_fixture(z)
    try:
        _check_rows(eng, z["thetas"], z["lb"], z["ub"], insts, name)
    finally:
        eng.close()


# ---- 3. shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 63, 64, 65, 512, 513, 1500])
def test_batch_sizes(W):
    z = load_golden("c0_mgii")
    insts = vo.instruments_from_fixture(z)
    base = z["thetas"]
    rows = base[np.arange(W) % len(base)]
    with engine_from_fixture(z) as eng:
        lp, g = eng.lnprob_grad(rows)
        lp0, g0 = eng.lnprob_grad(base)
        _check_rows(eng, base, z["lb"], z["ub"], insts, "c0_mgii")
    # a row's bits do not depend on the batch it is in
    assert _same_bits(g, g0[np.arange(W) % len(base)])
    np.testing.assert_allclose(lp, lp0[np.arange(W) % len(base)], rtol=LNPROB_RTOL, equal_nan=True)


def _tail_engine(shapes):
    import test_gpu_tile_tails as tt
    e, insts = tt._engine(tuple(shapes))
    return tt, e, insts


# P for every K: last pixel block (256) and last chunk (2048) of the adjoint launches empty, one pixel, full; and P mod 6 over 0..5
@pytest.mark.parametrize("K,Ps", [(1, (1500, 2048, 2049)), (9, (1501, 2304, 2305)), (17, (1502, 4095, 4097)), (33, (1503, 2111, 2561)),
                                  (65, (1504, 2303, 4096)), (2049, (2305, 2500, 4099))])
def test_tap_counts_and_tails(K, Ps):
    for P in Ps:
        tt, e, insts = _tail_engine([(K, P)])
        try:
            _check_rows(e, tt._rows(3, 100 + P), tt.LB, tt.UB, insts, "K=%d P=%d (P %% 6 = %d)" % (K, P, P % 6))
        finally:
            e.close()


@pytest.mark.parametrize("K,P", [(17, 7), (9, 1), (65, 40), (2049, 300), (1, 1)])
def test_fewer_pixels_than_taps(K, P):
    tt, e, insts = _tail_engine([(K, P)])
    try:
        _check_rows(e, tt._rows(4, 7 * K + P), tt.LB, tt.UB, insts, "K=%d P=%d" % (K, P))
    finally:
        e.close()


# ---- 4. row isolation, determinism ---------------------------------------------------------------------------------------
def test_row_isolation_and_determinism():
    z = load_golden("c3_mini")
    good = np.array([t for t in z["thetas"] if np.isfinite(vo.lnprob(t, z["lb"], z["ub"], vo.instruments_from_fixture(z)))])
    assert len(good) >= 3
    nan_row = good[0].copy(); nan_row[3] = np.nan
    out_row = good[1].copy(); out_row[0] = z["ub"][0] + 1.0
    batch = np.vstack([nan_row, good[0], out_row, good[1], nan_row, out_row, good[2]])
    where = [1, 3, 6]
    with engine_from_fixture(z) as eng:
        lp, g = eng.lnprob_grad(batch)
        lp2, g2 = eng.lnprob_grad(batch)
        assert _same_bits(lp, lp2) and _same_bits(g, g2)                         # two calls: identical bits
        assert np.isnan(lp[0]) and np.isneginf(lp[2]) and np.all(np.isnan(g[[0, 2, 4, 5]]))
        for k, w in enumerate(where):                                            # finite rows: as when evaluated alone
            lp1, g1 = eng.lnprob_grad(good[k])
            assert _same_bits(g[w], g1[0]) and _same_bits(lp[w:w + 1], lp1)
        perm = np.random.default_rng(3).permutation(len(batch))
        lpp, gp = eng.lnprob_grad(batch[perm])
        assert _same_bits(lpp, lp[perm]) and _same_bits(gp, g[perm])             # a permuted batch: the permuted result


def test_zero_error_instrument_gives_nan_rows_and_spares_the_other_context():
    z = load_golden("c0_mgii")
    import rbvfit_amd
    g_ = lambda k: z["G__" + k]
    w = g_("inv_sigma2").copy(); lw = g_("log_inv_sigma2").copy()
    w[100] = np.inf; lw[100] = np.inf                                            # error = 0 at one pixel
    bad = rbvfit_amd.Engine(0)
    bad.set_bounds(z["lb"], z["ub"])
    bad.add_instrument(g_("wave"), g_("flux"), w, lw, g_("lambda0"), g_("gamma"), g_("f"), g_("zfac"), g_("N_idx"), g_("b_idx"),
                       g_("v_idx"), taps=g_("taps"), lsf_mode=int(g_("lsf_mode")), voigt_method=int(g_("voigt_method")))
    with bad, engine_from_fixture(z) as eng:
        lp0, g0 = eng.lnprob_grad(z["thetas"])
        lpb, gb = bad.lnprob_grad(z["thetas"])
        ref = bad.lnprob(z["thetas"])
        assert not np.any(np.isfinite(ref))
        assert np.array_equal(np.isnan(lpb), np.isnan(ref)) and np.array_equal(np.isneginf(lpb), np.isneginf(ref))
        assert np.all(np.isnan(gb))
        lp1, g1 = eng.lnprob_grad(z["thetas"])
        assert _same_bits(lp0, lp1) and _same_bits(g0, g1)


# ---- 5. tied parameters --------------------------------------------------------------------------------------------------
def test_four_lines_share_one_b():
    import rbvfit_amd
    lam0 = np.array([2600.1729, 2586.650, 2382.765, 2344.214])
    gam = np.array([2.70e8, 2.72e8, 3.13e8, 2.68e8])
    f = np.array([0.239, 0.0691, 0.320, 0.114])
    zf = np.full(4, 1.3)
    Ni, bi, vi = np.arange(4), np.full(4, 4), np.arange(5, 9)
    theta = np.array([13.4, 13.9, 13.2, 13.7, 18.0, -20.0, 15.0, 40.0, -55.0])
    lb = np.array([10.0] * 4 + [1.0] + [-300.0] * 4)
    ub = np.array([18.0] * 4 + [100.0] + [300.0] * 4)
    taps = vo.gaussian_taps(4.0)
    data = vo.OracleModelData(lam0, gam, f, zf, Ni, bi, vi, taps, vo.LSF_SCIPY_NEAREST)
    P = 3000
    wave = np.linspace(3040.0, 3390.0, P)
    rng = np.random.default_rng(9)
    err = rng.uniform(0.03, 0.06, P)
    flux = vo.model_flux(data, theta, wave) + rng.normal(0, 1, P) * err
    oi = vo.OracleInstrument.from_error(data, wave, flux, err)
    rows = np.clip(theta + rng.normal(0, 1, (5, 9)) * np.array([0.1] * 4 + [2.0] + [4.0] * 4), lb, ub)
    with rbvfit_amd.Engine(0) as eng:
        eng.set_bounds(lb, ub)
        eng.add_instrument(wave, flux, oi.inv_sigma2, oi.log_inv_sigma2, lam0, gam, f, zf, Ni, bi, vi, taps=taps,
                           lsf_mode=vo.LSF_SCIPY_NEAREST, voigt_method=0)
        _check_rows(eng, rows, lb, ub, [oi], "four lines, one b")


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,text", [("c0_mgii_fast", "voigt_method 'fast'"), ("nan_wave_gauss", "NaN wavelength"),
                                       ("nan_wave_custom", "NaN wavelength")])
def test_refused_instruments(name, text):
    from rbvfit_amd._lib import RbvfitAmdError, VP_EINVAL
    z = load_golden(name)
    with engine_from_fixture(z) as eng:
        with pytest.raises(RbvfitAmdError, match=text) as ei:
            eng.lnprob_grad(z["thetas"])
        assert ei.value.code == VP_EINVAL
        got = eng.lnprob(z["thetas"])                                            # the context stays usable
        ref = vo.lnprob_batch(z["thetas"], z["lb"], z["ub"], vo.instruments_from_fixture(z))
        fin = np.isfinite(ref)
        assert np.array_equal(np.isfinite(got), fin)
        np.testing.assert_allclose(got[fin], ref[fin], rtol=LNPROB_RTOL, atol=1e-7)


def test_host_callable_instrument_refused_in_vfit():
    import test_gpu_adapters as ta
    from rbvfit_amd import vfit as mc
    fit, z = ta._fitter()
    inst = {"G": {"model": lambda th, wv: np.ones_like(wv), "wave": z["G__wave"], "flux": z["G__flux"],
                  "error": 1.0 / np.sqrt(z["G__inv_sigma2"])}}
    host = mc.vfit(inst, z["theta_true"], z["lb"], z["ub"], no_of_Chain=16, no_of_steps=2)
    try:
        with pytest.raises(NotImplementedError, match="host-callable"):
            host.lnprob_grad(z["theta_true"])
        with pytest.raises(NotImplementedError, match="host-callable"):
            host.fit_quick(grad="analytic")
        with pytest.raises(ValueError):
            fit.optimize_guess(z["theta_true"], grad="automatic")
    finally:
        host.close(); fit.close()


# ---- 7. device entry -----------------------------------------------------------------------------------------------------
def test_device_entry_equals_host_entry():
    import torch
    z = load_golden("c3_mini")
    with engine_from_fixture(z) as eng:
        lp, g = eng.lnprob_grad(z["thetas"])
        dev = torch.device("cuda", 0)
        th = torch.as_tensor(np.ascontiguousarray(z["thetas"]), device=dev)
        d_lp = torch.empty(th.shape[0], dtype=torch.float64, device=dev)
        d_g = torch.empty(th.shape, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        eng.lnprob_grad_device(th.data_ptr(), d_lp.data_ptr(), d_g.data_ptr(), th.shape[0], 0)
        torch.cuda.synchronize()                                                 # (stream 0 = the context's own stream)
        assert _same_bits(d_lp.cpu().numpy(), lp) and _same_bits(d_g.cpu().numpy(), g)


# ---- 8. consumers --------------------------------------------------------------------------------------------------------
def test_optimisers_with_the_analytic_gradient():
    """The analytic runs must reach an lnprob not lower than the finite-difference runs reach (values of the objective are
    compared, not theta).  Iteration counts are printed, and recorded in profiles/grad_notes.md; no threshold on them."""
    import scipy.optimize as op
    import test_gpu_adapters as ta
    fit, z = ta._fitter()
    try:
        frac = 0.05                                                              # of the fixture's box, per component
        start = np.clip(z["theta_true"] + frac * (z["ub"] - z["lb"]) * np.array([0.4, -0.3, 0.2, -0.2, 0.1, -0.1]), z["lb"], z["ub"])
        calls = {"n": 0}
        real = op.minimize

        def counting(*a, **k):
            res = real(*a, **k)
            calls["n"] = (res.nit, res.nfev)
            return res
        op.minimize = counting
        try:
            t_fd = fit.optimize_guess(start, grad="fd"); n_fd = calls["n"]
            t_an = fit.optimize_guess(start, grad="analytic"); n_an = calls["n"]
            fit.theta = start
            q_fd, _ = fit.fit_quick(grad="fd"); m_fd = calls["n"]
            q_an, e_an = fit.fit_quick(grad="analytic"); m_an = calls["n"]
        finally:
            op.minimize = real
        lp = fit.lnprob(np.vstack([t_fd, t_an, q_fd, q_an]))
        print("optimize_guess: lnprob fd %.6f (nit, nfev = %s), analytic %.6f (%s)" % (lp[0], n_fd, lp[1], n_an))
        print("fit_quick:      lnprob fd %.6f (nit, nfev = %s), analytic %.6f (%s)" % (lp[2], m_fd, lp[3], m_an))
        assert np.all(np.isfinite(lp)) and np.all(np.isfinite(e_an))
        assert lp[1] >= lp[0] and lp[3] >= lp[2]
    finally:
        fit.close()
