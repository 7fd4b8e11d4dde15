"""LSF tile tails and row isolation on the GPU vs the oracle.

A lane of lsf_block6 produces six consecutive outputs; the lanes past a tile's end repeat its last group of six, and the
taps are zero-padded to whole groups of eight.  So the chi^2 / flux lanes read flux words behind a tile's last evaluated
pixel, and the outputs that do not exist enter chi^2 with weight zero -- which keeps the sum finite only where those
words are.  These tests put the last tile of every launch form on every residue of its output count mod 6, for LSF
lengths on both sides of the tap-group and tile-width rules (capi_setup.inc), and check:
  * lnprob and model_flux against the oracle, and that no flux lane writes past the last row;
  * that a finite row's lnprob does not depend on the rows around it (NaN neighbours, LDS left dirty by other work);
  * the generic launch's slot form, whose workgroups walk several walkers in a row through one LDS block;
  * the device slice sampler on the full-size two-instrument workload."""
import functools

import numpy as np
import pytest

from conftest import FLUX_ATOL, LNPROB_RTOL, LNPROB_ATOL

pytestmark = pytest.mark.gpu

RB = 3                        # vp::RB: 64-pixel chunks per wave pass
LSF_PX = 6                    # vp::LSF_PX: outputs per lane
WAVE_LO, WAVE_HI = 3040.0, 3390.0
FEII = [2600.1729, 2586.650, 2382.765, 2344.214]
THETA = np.array([13.6, 13.1, 22.0, 35.0, -30.0, 45.0])        # N (2), b (2), v (2): 8 lines (FeII x 2 components)
LB = np.array([10.0, 10.0, 1.0, 1.0, -300.0, -300.0])
UB = np.array([18.0, 18.0, 150.0, 150.0, 300.0, 300.0])
SWEEP_K = [1, 3, 9, 17, 23, 33, 41, 65, 101, 265]           # 265 > 257: the wide-span rule


# ---- the tile geometry of vp_add_instrument (capi_setup.inc), mirrored -----------------------------------------------
def _geometry(K, P, span_opt=0):
    """{"nwaves", "dev", "dev_s", "dev_w"}: (span, TP, ntiles) of the two-pass tiles, the one-pass tiles and the walker
    kernel's tiles (None where the walker kernel has no geometry for the instrument)."""
    nwaves = 1 if K <= 33 else 2 if K <= 65 else 4
    span = 2 * 64 * RB * nwaves
    if span_opt > 0:
        span = max(64, (span_opt // 64) * 64)
    if K > 257:
        span, nwaves = min(8192, ((4 * K + 63) // 64) * 64), 4
    if P + K - 1 < span:
        span = max(64, ((P + K - 1 + 63) // 64) * 64)
    geo = lambda s: (s, s - (K - 1), -(-P // (s - (K - 1))))
    dev = geo(span)
    span_s = 64 * RB * nwaves
    dev_s = geo(span_s) if span_s < span and span_s - (K - 1) >= 64 else dev
    if nwaves == 1:
        dev_w = dev
    else:
        dev_w = geo(2 * 64 * RB) if 2 * 64 * RB - (K - 1) >= 64 and span_opt == 0 else None
    return dict(nwaves=nwaves, dev=dev, dev_s=dev_s, dev_w=dev_w)


def _last_nout(g, P):
    span, TP, nt = g
    return P - (nt - 1) * TP


def _pick_p(K, which, residue, span_opt=0, single=False, start=None):
    """The smallest pixel count from `start` on whose last `which` tile has nout % 6 == residue (at least two tiles of that
    geometry, or exactly one with `single`)."""
    P = start or 40
    while P < 20000:
        g = _geometry(K, P, span_opt)
        t = g[which]
        if t is not None and (t[2] == 1) == single and _last_nout(t, P) % LSF_PX == residue:
            return P
        P += 1
    raise AssertionError("no pixel count for K=%d %s residue %d" % (K, which, residue))


def _sweep_shapes(K):
    """Pixel counts for K: the two-pass tiles' last tile on every residue, the one-pass and walker tiles' on the two that
    reach furthest (1, 2), and a single-tile instrument."""
    g0 = _geometry(K, 100000)
    out = set()
    for r in range(LSF_PX):
        out.add(_pick_p(K, "dev", r, start=g0["dev"][1] + g0["dev"][1] // 3))
    for which in ("dev_s", "dev_w"):
        if g0[which] is not None and g0[which] != g0["dev"]:
            for r in (1, 2):
                out.add(_pick_p(K, which, r, start=g0[which][1] + g0[which][1] // 3))
    out.add(_pick_p(K, "dev", 2, single=True, start=max(LSF_PX + 1, 60)))
    return sorted(out)


# ---- models, instruments, oracle ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model_data(K):
    from rbvfit_amd.model import FitConfiguration, VoigtModel
    cfg = FitConfiguration()
    cfg.add_system(0.3, "FeII", FEII, 2)
    if K == 1:
        model = VoigtModel(cfg, FWHM=None)
    else:
        j = np.arange(K) - K // 2
        model = VoigtModel(cfg, kernel_taps=np.exp(-0.5 * (j / max(1.0, K / 7.0)) ** 2) + 1e-3)
    data = model.compile().data
    assert data.n_lines == 8 and (K == 1 or data.taps.size == K)
    return data


def _oracle_data(data):
    from oracle import voigt_oracle as vo
    return vo.OracleModelData(data.atomic_lambda0, data.atomic_gamma, data.atomic_f, data.z_factors, data.N_indices,
                              data.b_indices, data.v_indices, data.taps if data.taps is not None else np.zeros(0),
                              data.lsf_mode, data.voigt_method)


@functools.lru_cache(maxsize=None)
def _instrument(K, P):
    from oracle import voigt_oracle as vo
    data = _model_data(K)
    od = _oracle_data(data)
    wave = np.linspace(WAVE_LO, WAVE_HI, P)
    rng = np.random.default_rng(1000 * P + K)
    err = rng.uniform(0.03, 0.08, P)
    flux = vo.model_flux(od, THETA, wave) + rng.normal(0.0, 1.0, P) * err
    return data, od, vo.OracleInstrument.from_error(od, wave, flux, err)


def _engine(shapes, lb=LB, ub=UB, options=()):
    import rbvfit_amd
    e = rbvfit_amd.Engine(0)
    for k, v in options:
        e.set_option(k, v)
    e.set_bounds(lb, ub)
    insts = []
    for K, P in shapes:
        data, od, oi = _instrument(K, P)
        e.add_instrument(oi.wave, oi.flux, oi.inv_sigma2, oi.log_inv_sigma2, **data.engine_kwargs())
        insts.append(oi)
    return e, insts


def _rows(W, seed):
    rng = np.random.default_rng(seed)
    th = THETA + rng.normal(0.0, 1.0, (W, THETA.size)) * np.array([0.15, 0.15, 3.0, 3.0, 6.0, 6.0])
    th[0] = THETA
    return np.clip(th, LB + 1e-9, UB - 1e-9)


# ---- the launch forms -----------------------------------------------------------------------------------------------
_KNOBS = ("walker", "walker_split", "geom", "finalize", "farfield", "tile_multi")
_DEFAULT = dict(walker=-1, walker_split=0, geom=-1, finalize=-1, farfield=-1, tile_multi=-1)


def _set(e, **kw):
    for k in _KNOBS:
        e.set_option(k, kw.get(k, _DEFAULT[k]))


def _forms(shapes, W, span_opt=0):
    """[(name, knobs, expected last_launch_kind or None, expected last_walker_split or None)] for an engine of `shapes` (same
    lines throughout): every form the engine has for a W-row batch.  An expectation of None: the mirror does not vouch
    for the form (the batch is still checked, whatever form it took)."""
    geos = [_geometry(K, P, span_opt) for K, P in shapes]
    forms = []
    walker_ok = all(g["dev_w"] is not None for g in geos) and sum(g["dev_w"][2] for g in geos) <= 8
    forms.append(("walker", dict(walker=1), "walker" if walker_ok else None, 0 if walker_ok else None))
    if len(shapes) == 1:
        g = geos[0]
        split_ok = walker_ok and g["nwaves"] == 1 and g["dev_s"][0] < g["dev"][0] and g["dev_s"][2] >= 2 and span_opt == 0
        for G in (-1, 2, 8):
            want = min(8 if G < 0 else G, g["dev_s"][2]) if split_ok else 0
            if want >= 2:
                forms.append(("walker_split%d" % G, dict(walker=1, walker_split=G), "walker", want))
    for geom in (0, 1):
        for fin in (0, 1):
            forms.append(("tiles_g%d_f%d" % (geom, fin), dict(walker=0, geom=geom, finalize=fin, farfield=0, tile_multi=0),
                          "tiles", None))
    forms.append(("tiles+farfield", dict(walker=0, geom=0, farfield=1, tile_multi=0), "tiles+farfield", None))
    forms.append(("tiles+farfield_g1", dict(walker=0, geom=1, farfield=1, tile_multi=0), "tiles+farfield", None))
    if len(shapes) >= 2:
        multi_ok = all(g["dev_w"] is not None for g in geos)
        for fin in (0, 1):
            forms.append(("tiles-multi_f%d" % fin, dict(walker=0, tile_multi=1, finalize=fin, farfield=0),
                          "tiles-multi" if multi_ok else None, None))
    return forms


def _run(e, forms, thetas):
    """{name: lnprob} of `thetas` through every form, each checked to have been the form it claims."""
    out = {}
    for name, knobs, kind, split in forms:
        _set(e, **knobs)
        out[name] = e.lnprob(thetas)
        if kind is not None:
            assert e.last_launch_kind == kind, (name, e.last_launch_kind)
        if split is not None:
            assert e.last_walker_split == split, (name, e.last_walker_split)
    _set(e)
    return out


def _check_flux(e, od, oi, thetas, walker_forms):
    """model_flux (convolved through the walker kernel's flux form and the tile launches, unconvolved) vs the oracle, and
    the device form into a buffer one row longer than the batch: the extra row keeps its sentinel."""
    import torch
    from oracle import voigt_oracle as vo
    W, P = thetas.shape[0], oi.wave.size
    ref = np.array([vo.model_flux(od, t, oi.wave) for t in thetas])
    ref_un = np.array([vo.model_flux(od, t, oi.wave, return_unconvolved=True) for t in thetas])
    d_th = torch.tensor(thetas, dtype=torch.float64, device="cuda")
    sentinel = -777.25
    for walker in walker_forms:
        _set(e, walker=walker)
        for conv, want in ((True, ref), (False, ref_un)):
            got = e.model_flux(0, thetas, convolved=conv)
            np.testing.assert_allclose(got, want, rtol=0, atol=FLUX_ATOL, err_msg="walker=%d convolved=%s" % (walker, conv))
            buf = torch.full(((W + 1) * P,), sentinel, dtype=torch.float64, device="cuda")
            e.model_flux_device(0, d_th.data_ptr(), buf.data_ptr(), W, convolved=conv,
                                stream_ptr=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            assert np.all(host[W * P:] == sentinel), "a flux lane wrote past the last row (walker=%d convolved=%s)" % (walker, conv)
            assert np.array_equal(host[:W * P].reshape(W, P), got), "device and host model_flux differ"
    _set(e)


# ---- a. residue sweep -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", SWEEP_K)
def test_last_tile_residues(K):
    from oracle import voigt_oracle as vo
    W = 6
    thetas = _rows(W, K)
    cases = [((K, P),) for P in _sweep_shapes(K)]
    span_opts = []
    if K in (9, 17, 41):
        # full tiles on the other even residues (TP = span - (K - 1) is even: K odd, span a multiple of 64)
        span_opts = [S for S in (320, 448, 512) if S - (K - 1) >= 64]
    seen = set()
    runs = [(shapes, 0) for shapes in cases] + [(((K, 1500),), S) for S in span_opts]
    for shapes, S in runs:
        e, insts = _engine(shapes, options=(("span", S),) if S else ())
        try:
            ref = vo.lnprob_batch(thetas, LB, UB, insts)
            assert np.all(np.isfinite(ref))
            got = _run(e, _forms(shapes, W, S), thetas)
            for name, r in got.items():
                np.testing.assert_allclose(r, ref, rtol=LNPROB_RTOL, atol=LNPROB_ATOL, err_msg="%s P=%d span=%d" % (name, shapes[0][1], S))
            g = _geometry(K, shapes[0][1], S)
            for which in ("dev", "dev_s", "dev_w"):
                if g[which] is not None:
                    seen.add((which, _last_nout(g[which], shapes[0][1]) % LSF_PX, g[which][2] == 1))
            walker_forms = (0, 1) if g["dev_w"] is not None and g["dev_w"][2] <= 8 else (0,)
            _check_flux(e, _oracle_data(_model_data(K)), insts[0], thetas[:3], walker_forms)
        finally:
            e.close()
    assert {r for w, r, single in seen if w == "dev" and not single} == set(range(LSF_PX))
    assert ("dev", 2, True) in seen


@pytest.mark.parametrize("Ks", [(9, 9), (17, 17), (41, 41), (9, 17, 41, 23)])
def test_last_tile_residues_multi(Ks):
    """Several instruments with the same lines: the walker kernel's two- / four-instrument forms and tile_kernel_multi,
    each instrument's last walker tile on residue 1 or 2."""
    from oracle import voigt_oracle as vo
    W = 6
    thetas = _rows(W, sum(Ks))
    shapes = []
    for i, K in enumerate(Ks):
        g0 = _geometry(K, 100000)
        shapes.append((K, _pick_p(K, "dev_w", 1 + i % 2, start=g0["dev_w"][1] + 1 + 37 * i)))
    e, insts = _engine(shapes)
    try:
        ref = vo.lnprob_batch(thetas, LB, UB, insts)
        got = _run(e, _forms(shapes, W), thetas)
        for name, r in got.items():
            np.testing.assert_allclose(r, ref, rtol=LNPROB_RTOL, atol=LNPROB_ATOL, err_msg=name)
    finally:
        e.close()


# ---- b. row isolation -----------------------------------------------------------------------------------------------
_DIRTY = {}


def _dirty_lds():
    """Leave NaN flux in the LDS of every CU: all-NaN batches through a wide-span (4-wave) instrument, as lnprob and as
    model_flux."""
    if "e" not in _DIRTY:
        _DIRTY["e"], _ = _engine([(101, 3000)])
    e = _DIRTY["e"]
    bad = np.tile(THETA, (512, 1))
    bad[:, 0] = np.nan
    _set(e, walker=0)
    r = e.lnprob(bad)
    assert np.all(np.isnan(r))
    assert np.all(np.isnan(e.model_flux(0, bad[:256])))
    _set(e)


@pytest.fixture(scope="module", autouse=True)
def _close_dirty():
    yield
    if "e" in _DIRTY:
        _DIRTY.pop("e").close()


def _isolation_shapes():
    out = []
    for r in (1, 2):
        g0 = _geometry(9, 100000)
        out.append(("K9_r%d" % r, ((9, _pick_p(9, "dev", r, start=g0["dev"][1] + 1)),)))
    out.append(("K9_c3", ((9, 8192),)))           # C3's instrument B: last tile nout = 296
    out.append(("K17", ((17, 1000),)))            # full tiles of 368 (two-pass) and 176 (one-pass) outputs: % 6 == 2
    out.append(("K41", ((41, 1500),)))            # two-wave tiles of 728: % 6 == 2
    out.append(("K17_K17", ((17, 1000), (17, _pick_p(17, "dev_w", 1, start=400)))))
    return out


@pytest.mark.parametrize("name,shapes", _isolation_shapes(), ids=[n for n, _ in _isolation_shapes()])
def test_finite_rows_ignore_nan_neighbours(name, shapes):
    from oracle import voigt_oracle as vo
    W = 24
    clean = _rows(W, 7)
    nan_rows = np.arange(W) % 3 == 1
    mixed = clean.copy()
    mixed[nan_rows, 0] = np.nan
    e, insts = _engine(shapes)
    try:
        ref = vo.lnprob_batch(clean[~nan_rows], LB, UB, insts)
        forms = _forms(shapes, W)
        got_clean = _run(e, forms, clean)
        got_mixed = _run(e, forms, mixed)
        _dirty_lds()
        got_dirty = _run(e, forms, mixed)
        for fname in got_clean:
            c = got_clean[fname]
            np.testing.assert_allclose(c[~nan_rows], ref, rtol=LNPROB_RTOL, atol=LNPROB_ATOL, err_msg=fname)
            for tag, m in (("mixed", got_mixed[fname]), ("dirty LDS", got_dirty[fname])):
                assert np.all(np.isnan(m[nan_rows])), (fname, tag)
                bad = np.flatnonzero(~(m[~nan_rows] == c[~nan_rows]))
                assert bad.size == 0, "%s (%s): finite rows %s differ from the clean batch: %s" % (
                    fname, tag, np.flatnonzero(~nan_rows)[bad].tolist(), m[~nan_rows][bad].tolist())
        if len(shapes) == 1:
            # model_flux: the finite rows of a mixed batch, after dirty LDS, are those of the clean batch
            for walker in (0, 1):
                _set(e, walker=walker)
                fc = e.model_flux(0, clean)
                _dirty_lds()
                _set(e, walker=walker)
                fm = e.model_flux(0, mixed)
                assert np.array_equal(fm[~nan_rows], fc[~nan_rows]) and np.all(np.isnan(fm[nan_rows]))
            _set(e)
    finally:
        e.close()


# ---- c. the generic launch's slot form ------------------------------------------------------------------------------
def test_generic_slots_isolate_walkers():
    """A prior box whose lower b bound lets the damping parameter exceed 0.1 sends flagged walkers to the generic launch;
    while no batch of the context has flagged one, that launch is GEN_SLOTS (64) workgroups per tile, each walking the walkers
    slot, slot + 64, ... through ONE LDS block.  Row i (flagged, NaN) goes right before row i + 64 (flagged, finite) in the
    same workgroup: the finite row must come out as the oracle's."""
    from oracle import voigt_oracle as vo
    lb = LB.copy()
    lb[2:4] = 0.0                               # needs_generic
    W, i = 128, 5
    quiet = _rows(W, 3)
    mixed = quiet.copy()
    mixed[[i, i + 64], 2] = 0.02                # a ~ 0.25: outside the fast domain
    mixed[i, 0] = np.nan
    shapes = ((17, 1000),)                      # full tiles: 368 outputs (two-pass), 176 (one-pass); both % 6 == 2
    ref = None
    for geom in (0, 1):                         # (a fresh context each: only its first flagged batch takes the slot form)
        e, insts = _engine(shapes, lb=lb, options=(("walker", 0), ("geom", geom)))
        try:
            if ref is None:
                ref = vo.lnprob_batch(mixed[[i + 64, i + 1]], lb, UB, insts)
            q = e.lnprob(quiet)                 # nothing flagged: the next batch's generic launch takes the slot form
            assert np.all(np.isfinite(q))
            got = e.lnprob(mixed)
            assert np.isnan(got[i])
            np.testing.assert_allclose(got[[i + 64, i + 1]], ref, rtol=LNPROB_RTOL, atol=LNPROB_ATOL, err_msg="geom %d" % geom)
            np.testing.assert_array_equal(np.delete(got, [i, i + 64]), np.delete(q, [i, i + 64]))
            again = e.lnprob(mixed)             # ... and the one-workgroup-per-walker form
            assert np.isnan(again[i])
            np.testing.assert_array_equal(np.delete(again, i), np.delete(got, i))
        finally:
            e.close()


# ---- d. the slice sampler on the full-size two-instrument workload ---------------------------------------------------
def test_slice_sampler_c3_full_ensemble():
    """The bench's c3_2048_walkers leg: 2 + 6 iterations of the device slice sampler on C3 (two instruments of 8192 pixels,
    9- and 101-tap LSFs) with its whole ensemble; every lnprob it keeps is finite and is the engine's and the oracle's."""
    from oracle import voigt_oracle as vo
    from rbvfit_amd.workloads import make_workload
    wl = make_workload("C3", walkers=2048)
    try:
        e = wl.engine
        r0 = e.slice_run(wl.thetas, 2, seed=1, store_chain=False)
        r1 = e.slice_run(r0["pos"], 6, lnprob=r0["lnprob"], seed=1, step0=2, mu=r0["mu"], tune=r0["tune"], store_chain=True)
        assert np.all(np.isfinite(r0["lnprob"])) and np.all(np.isfinite(r1["lnprob"]))
        assert np.all(np.isfinite(r1["chain_lnprob"]))
        np.testing.assert_allclose(r1["lnprob"], e.lnprob(r1["pos"]), rtol=LNPROB_RTOL, atol=LNPROB_ATOL)
        insts = [vo.OracleInstrument.from_error(_oracle_data(t), w, f, err) for t, (w, f, err) in zip(wl.tables, wl.spectra)]
        rows = np.linspace(0, len(r1["pos"]) - 1, 16).astype(int)
        ref = vo.lnprob_batch(r1["pos"][rows], wl.lb, wl.ub, insts)
        np.testing.assert_allclose(r1["lnprob"][rows], ref, rtol=LNPROB_RTOL, atol=LNPROB_ATOL)
    finally:
        wl.engine.close()
