"""GPU tests of the model Jacobian and the Fisher matrix (vp_model_flux_jacobian, vp_fisher_batch*) against the CPU yardstick
tests/fisher_reference.py.

Tolerances: |J - J_ref| <= 1e-10 A (the project's GRAD_RTOL carried to the same kind of sum; A = the sum of the absolute values
of the terms of a Jacobian entry) and |F - F_ref| <= 2e-10 FA (product rule: dF <= sum w (|dJ_j| |J_k| + |J_j| |dJ_k|)).
Measured worst ratios: profiles/fisher_notes.md."""
import warnings

import numpy as np
import pytest

from conftest import load_golden, LNPROB_RTOL
from helpers import engine_from_fixture, fixture_instruments
from oracle import voigt_oracle as vo
import grad_reference as gr
import fisher_reference as fr
from test_gpu_grad import PARITY, GRAD_RTOL, _same_bits

pytestmark = pytest.mark.gpu

JAC_RTOL = GRAD_RTOL         # x A
FISHER_RTOL = 2e-10          # x FA
_REF = {}                    # name -> (in-box rows, [F], [FA]): filled by whichever parity test runs first, never modified


def _inbox(z, insts):
    return np.array([t for t in z["thetas"] if np.isfinite(vo.lnprob(t, z["lb"], z["ub"], insts))])


def _fisher_ref(name, z, insts):
    if name not in _REF:
        rows = _inbox(z, insts)
        pairs = [fr.fisher(t, insts) for t in rows]
        _REF[name] = (rows, [p[0] for p in pairs], [p[1] for p in pairs])
    return _REF[name]


# ---- 1. parity on the fixtures -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PARITY)
def test_jacobian_parity(name):
    z = load_golden(name)
    insts = vo.instruments_from_fixture(z)
    rows = _inbox(z, insts)
    assert len(rows) >= 1
    worst = {True: 0.0, False: 0.0}
    F = [np.zeros((rows.shape[1],) * 2) for _ in rows]
    FA = [np.zeros((rows.shape[1],) * 2) for _ in rows]
    with engine_from_fixture(z) as eng:
        for i, inst in enumerate(insts):
            for conv in (True, False):
                got = eng.model_flux_jacobian(i, rows, convolved=conv)
                assert got.shape == (len(rows), rows.shape[1], inst.wave.size)
                for w, t in enumerate(rows):
                    J, A = fr.jacobian(t, inst, convolved=conv)
                    if conv:
                        F[w] += (J * inst.inv_sigma2[None, :]) @ J.T
                        FA[w] += (A * inst.inv_sigma2[None, :]) @ A.T
                    err = np.abs(got[w] - J)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        ratio = np.where(err > 0, err / A, 0.0)
                    worst[conv] = max(worst[conv], float(ratio.max()))
                    assert np.all(err <= JAC_RTOL * A), "%s inst %d row %d convolved=%s: worst |dJ|/A = %.3e" % (name, i, w, conv, ratio.max())
    _REF.setdefault(name, (rows, F, FA))
    print("%s: %d rows, worst |J - J_ref| / A = %.3e convolved, %.3e unconvolved" % (name, len(rows), worst[True], worst[False]))


@pytest.mark.parametrize("name", PARITY)
def test_fisher_parity(name):
    z = load_golden(name)
    insts = vo.instruments_from_fixture(z)
    rows, Fr, FAr = _fisher_ref(name, z, insts)
    with engine_from_fixture(z) as eng:
        lp, F = eng.fisher(rows)
        ref_lp = eng.lnprob(rows)
    D = rows.shape[1]
    assert lp.shape == (len(rows),) and F.shape == (len(rows), D, D)
    assert np.all(np.abs(lp - ref_lp) <= LNPROB_RTOL * np.abs(ref_lp))
    worst = 0.0
    for w in range(len(rows)):
        assert _same_bits(F[w], F[w].T), "%s row %d: F is not symmetric to the bit" % (name, w)
        err = np.abs(F[w] - Fr[w])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err > 0, err / FAr[w], 0.0)
        worst = max(worst, float(ratio.max()))
        assert np.all(err <= FISHER_RTOL * FAr[w]), "%s row %d: worst |dF|/FA = %.3e" % (name, w, ratio.max())
    print("%s: %d rows, worst |F - F_ref| / FA = %.3e" % (name, len(rows), worst))


# P for every K: last pixel block (256), last convolution tile (2048), last Fisher chunk (512) and last staged 64 pixels empty, one
# pixel, full; fewer pixels than taps
@pytest.mark.parametrize("K,Ps", [(1, (1, 513)), (9, (1, 2049)), (65, (40, 2048, 2113)), (2049, (300, 2305, 4099))])
def test_tap_counts_and_tails(K, Ps):
    import test_gpu_tile_tails as tt
    for P in Ps:
        e, insts = tt._engine(((K, P),))
        try:
            rows = tt._rows(2, 100 + P)
            got = e.model_flux_jacobian(0, rows)
            lp, F = e.fisher(rows)
            for w, t in enumerate(rows):
                J, A = fr.jacobian(t, insts[0])
                Fr, FAr = fr.fisher(t, insts)
                assert np.all(np.abs(got[w] - J) <= JAC_RTOL * A), "K=%d P=%d row %d: Jacobian" % (K, P, w)
                assert np.all(np.abs(F[w] - Fr) <= FISHER_RTOL * FAr), "K=%d P=%d row %d: Fisher" % (K, P, w)
                assert _same_bits(F[w], F[w].T)
        finally:
            e.close()


# ---- 2. against the gradient path ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c0_mgii", "c3_mini"])
def test_jacobian_contracts_to_the_gpu_gradient(name):
    z = load_golden(name)
    insts = vo.instruments_from_fixture(z)
    rows = _inbox(z, insts)[:4]
    with engine_from_fixture(z) as eng:
        _, g = eng.lnprob_grad(rows)
        acc = np.zeros_like(rows)
        for i, inst in enumerate(insts):
            J = eng.model_flux_jacobian(i, rows)
            m = eng.model_flux(i, rows)
            acc += np.einsum("wkp,wp->wk", J, inst.inv_sigma2[None, :] * (inst.flux[None, :] - m))
    worst = 0.0
    for w, t in enumerate(rows):
        _, _, S = gr.lnlike_grad(t, insts)
        worst = max(worst, float(np.max(np.abs(acc[w] - g[w]) / S)))
        assert np.all(np.abs(acc[w] - g[w]) <= 2e-10 * S)
    print("%s: worst |J^T q - grad| / S = %.3e" % (name, worst))


# ---- 3. lnprob, invalid rows, batches, determinism -----------------------------------------------------------------------
def test_invalid_rows_get_nan_blocks_and_spare_their_neighbours():
    z = load_golden("c3_mini")
    good = _inbox(z, vo.instruments_from_fixture(z))
    assert len(good) >= 3
    nan_row = good[0].copy(); nan_row[3] = np.nan
    out_row = good[1].copy(); out_row[0] = z["ub"][0] + 1.0
    batch = np.vstack([nan_row, good[0], out_row, good[1], nan_row, out_row, good[2]])
    where = [1, 3, 6]
    with engine_from_fixture(z) as eng:
        lp, F = eng.fisher(batch)
        lp2, F2 = eng.fisher(batch)
        ref = eng.lnprob(batch)
        assert _same_bits(lp, lp2) and _same_bits(F, F2)                         # two calls: identical bits
        assert np.isnan(lp[0]) and np.isneginf(lp[2]) and np.all(np.isnan(F[[0, 2, 4, 5]]))
        assert np.array_equal(np.isnan(lp), np.isnan(ref)) and np.array_equal(np.isneginf(lp), np.isneginf(ref))
        fin = np.isfinite(ref)
        assert np.all(np.abs(lp[fin] - ref[fin]) <= LNPROB_RTOL * np.abs(ref[fin])) and np.all(np.isfinite(F[fin]))
        lpg, Fg = eng.fisher(good[:3])                                           # a batch without the invalid rows
        assert _same_bits(F[where], Fg) and _same_bits(lp[where], lpg)
        for k, w in enumerate(where):                                            # ... and each row alone
            lp1, F1 = eng.fisher(good[k])
            assert _same_bits(F[w], F1[0]) and _same_bits(lp[w:w + 1], lp1)


def test_non_finite_lnlike_gives_nan_blocks():
    import rbvfit_amd
    z = load_golden("c0_mgii")
    g_ = lambda k: z["G__" + k]
    w = g_("inv_sigma2").copy(); lw = g_("log_inv_sigma2").copy()
    w[100] = np.inf; lw[100] = np.inf                                            # error = 0 at one pixel
    bad = rbvfit_amd.Engine(0)
    bad.set_bounds(z["lb"], z["ub"])
    bad.add_instrument(g_("wave"), g_("flux"), w, lw, g_("lambda0"), g_("gamma"), g_("f"), g_("zfac"), g_("N_idx"), g_("b_idx"),
                       g_("v_idx"), taps=g_("taps"), lsf_mode=int(g_("lsf_mode")), voigt_method=int(g_("voigt_method")))
    with bad:
        lp, F = bad.fisher(z["thetas"])
        ref = bad.lnprob(z["thetas"])
        assert not np.any(np.isfinite(ref))
        assert np.array_equal(np.isnan(lp), np.isnan(ref)) and np.array_equal(np.isneginf(lp), np.isneginf(ref))
        assert np.all(np.isnan(F))


@pytest.mark.parametrize("W", [1, 2, 63, 65, 513])
def test_batch_sizes(W):
    z = load_golden("c0_mgii")
    base = z["thetas"]
    pick = np.arange(W) % len(base)
    with engine_from_fixture(z) as eng:
        lp0, F0 = eng.fisher(base)
        lp, F = eng.fisher(base[pick])
    assert _same_bits(F, F0[pick])                                               # a row's bits do not depend on its batch
    np.testing.assert_allclose(lp, lp0[pick], rtol=LNPROB_RTOL, equal_nan=True)


def test_device_entry_equals_host_entry():
    import torch
    z = load_golden("c3_mini")
    with engine_from_fixture(z) as eng:
        lp, F = eng.fisher(z["thetas"])
        dev = torch.device("cuda", 0)
        th = torch.as_tensor(np.ascontiguousarray(z["thetas"]), device=dev)
        W, D = th.shape
        d_lp = torch.empty(W, dtype=torch.float64, device=dev)
        d_F = torch.empty((W, D, D), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        eng.fisher_device(th.data_ptr(), d_lp.data_ptr(), d_F.data_ptr(), W, 0)
        torch.cuda.synchronize()                                                 # (stream 0 = the context's own stream)
        assert _same_bits(d_lp.cpu().numpy(), lp) and _same_bits(d_F.cpu().numpy(), F)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,text", [("c0_mgii_fast", "voigt_method 'fast'"), ("nan_wave_gauss", "NaN wavelength"),
                                       ("nan_wave_custom", "NaN wavelength")])
def test_refused_instruments(name, text):
    from rbvfit_amd._lib import RbvfitAmdError, VP_EINVAL
    z = load_golden(name)
    with engine_from_fixture(z) as eng:
        for call, entry in ((lambda: eng.fisher(z["thetas"]), "vp_fisher_batch"),
                            (lambda: eng.model_flux_jacobian(0, z["thetas"]), "vp_model_flux_jacobian")):
            with pytest.raises(RbvfitAmdError, match=text) as ei:
                call()
            assert ei.value.code == VP_EINVAL and entry in str(ei.value)
        got = eng.lnprob(z["thetas"])                                            # the context stays usable
        ref = vo.lnprob_batch(z["thetas"], z["lb"], z["ub"], vo.instruments_from_fixture(z))
        fin = np.isfinite(ref)
        assert np.array_equal(np.isfinite(got), fin)
        np.testing.assert_allclose(got[fin], ref[fin], rtol=LNPROB_RTOL, atol=1e-7)


def _fitter_from_fixture(name):
    """A vfit on the fixture's own tables and spectra, started at its first in-box row."""
    from rbvfit_amd import vfit as mc
    from rbvfit_amd.model import CompiledModelData
    z = load_golden(name)
    insts = vo.instruments_from_fixture(z)
    D = len(z["lb"])
    data = {}
    for inst in fixture_instruments(z):
        g = lambda k: z[f"{inst}__{k}"]
        tables = CompiledModelData(g("lambda0"), g("gamma"), g("f"), g("zfac"), g("N_idx"), g("b_idx"), g("v_idx"), g("taps"),
                                   int(g("lsf_mode")), len(g("lambda0")), D // 3, "wofz")
        data[inst] = {"model": tables, "wave": g("wave"), "flux": g("flux"), "error": 1.0 / np.sqrt(g("inv_sigma2"))}
    start = _inbox(z, insts)[0]
    return mc.vfit(data, start, z["lb"], z["ub"], no_of_Chain=16, no_of_steps=2), z, insts, start


def test_host_callable_instrument_refused_in_vfit():
    from rbvfit_amd import vfit as mc
    z = load_golden("c0_mgii")
    inst = {"G": {"model": lambda th, wv: np.ones_like(wv), "wave": z["G__wave"], "flux": z["G__flux"],
                  "error": 1.0 / np.sqrt(z["G__inv_sigma2"])}}
    host = mc.vfit(inst, z["theta_true"], z["lb"], z["ub"], no_of_Chain=16, no_of_steps=2)
    try:
        for call in (lambda: host.fisher(z["theta_true"]), lambda: host.covariance(z["theta_true"]),
                     lambda: host.estimate_parameter_errors(z["theta_true"], method="fisher"), lambda: host.fit_quick(errors="fisher")):
            with pytest.raises(NotImplementedError, match="host-callable"):
                call()
        with pytest.raises(ValueError):
            host.fit_quick(errors="hessian")
    finally:
        host.close()


# ---- 5. consumers --------------------------------------------------------------------------------------------------------
def test_covariance_against_the_inverse_of_the_yardstick():
    fit, z, insts, start = _fitter_from_fixture("c0_mgii")
    try:
        cov = fit.covariance(start)
        lp, F = fit.fisher(start)
        assert np.isfinite(lp) and F.shape == (6, 6)
        err = fit.estimate_parameter_errors(start, method="fisher")
    finally:
        fit.close()
    Fr, _ = fr.fisher(start, insts)
    ref = np.linalg.inv(Fr)
    cond = fr.scaled_condition(Fr)
    scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
    ratio = np.abs(cov - ref) / scale
    print("c0_mgii: cond(C) = %.3f, worst |cov - inv(F_ref)| / sqrt(cov_jj cov_kk) = %.3e (bound %.3e)" % (cond, ratio.max(), cond * 4e-10))
    assert np.all(ratio <= cond * 4e-10)
    assert _same_bits(err, np.sqrt(np.diag(cov)))


def test_fit_quick_with_fisher_errors():
    fit, z, insts, start = _fitter_from_fixture("c0_mgii")
    try:
        q0, e0 = fit.fit_quick()                                                 # defaults: what they were
        assert not hasattr(fit, "theta_best_cov")
        assert _same_bits(e0, fit.estimate_parameter_errors(q0, start))
        qc, ec = fit.fit_quick(errors="curvature")
        assert _same_bits(qc, q0) and _same_bits(ec, e0)
        qf, ef = fit.fit_quick(errors="fisher")
        assert _same_bits(qf, q0)                                                # the same optimisation
        assert np.all(np.isfinite(ef)) and np.all(ef > 0)
        assert fit.theta_best_cov is not None and fit.theta_best_cov.shape == (6, 6)
        assert _same_bits(ef, np.sqrt(np.diag(fit.theta_best_cov))) and _same_bits(fit.theta_best_error, ef)
        assert _same_bits(fit.theta_best_cov, fit.covariance(qf))
        print("c0_mgii fit_quick: curvature errors %s\n                   fisher errors    %s" % (e0, ef))
    finally:
        fit.close()


def test_fit_quick_falls_back_on_a_singular_fisher_matrix():
    fit, z, insts, start = _fitter_from_fixture("c2_window")
    try:
        with pytest.raises(ValueError, match="not constrained by the data"):
            fit.covariance(start)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            q, e = fit.fit_quick(grad="analytic", errors="fisher")
        assert any("Fisher errors not available" in str(w.message) for w in rec)
        assert fit.theta_best_cov is None
        assert _same_bits(e, fit.estimate_parameter_errors(q, start))            # the curvature errors
    finally:
        fit.close()


# ---- 6. compiler output --------------------------------------------------------------------------------------------------
def test_fisher_kernels_use_no_scratch(tmp_path):
    from test_kernel_resources import _metadata
    meta = _metadata(tmp_path)
    mine = {k: v for k, v in meta.items() if k.startswith("vp::fisher_")}
    assert sorted(k.split("(")[0] for k in mine) == ["vp::fisher_block_kernel", "vp::fisher_conv_kernel", "vp::fisher_reduce_kernel",
                                                     "vp::fisher_rows_kernel"]
    for k, m in mine.items():
        print("%-28s vgpr %3d  sgpr %3d  lds %5d B  scratch %d B  spills v/s %d/%d" % (k.split("(")[0][4:], m["vgpr"], m["sgpr"], m["lds"],
                                                                                       m["scratch"], m["vgpr_spill"], m["sgpr_spill"]))
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, k
