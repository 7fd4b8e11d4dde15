"""walker_kernel's deals of a walker's tiles to the waves of its workgroup (option "walker_perm": 0 wave k takes tile k, 1 the
cost deal of batches with at most one workgroup per compute unit, 2 the grid-order deal of batches that put several on one).
Tile sums meet in LDS by TILE index, so lnprob and the sampler's chain must not depend on the deal by a single bit."""
import numpy as np
import pytest

from conftest import load_golden
from helpers import engine_from_fixture

pytestmark = pytest.mark.gpu

DEALS = (0, 1, 2)
FIXTURES = ["c0_mgii", "c0_mgii_strong", "ragged_1000", "tiny_7px", "one_px"]


def _rows(z, W):
    """W rows of the fixture's batch with a row below the prior box (-inf) and a NaN row among them (W >= 3)."""
    th = np.ascontiguousarray(z["thetas"][np.arange(W) % len(z["thetas"])], dtype=np.float64)
    if W >= 3:
        th[1, 0] = z["lb"][0] - 1.0
        th[2, -1] = np.nan
    return th


def _lnprob_device(eng, th):
    import torch
    d_th = torch.from_numpy(th).cuda()
    d_out = torch.full((len(th),), 12345.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng.lnprob_device(d_th.data_ptr(), d_out.data_ptr(), len(th), stream.cuda_stream)
    stream.synchronize()
    return d_out.cpu().numpy()


def _by_deal(eng, th):
    out = {}
    for mode in DEALS:
        eng.set_option("walker_perm", mode)
        out[mode] = _lnprob_device(eng, th)
        assert eng.last_launch_kind == "walker"
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_lnprob_does_not_depend_on_the_deal(name):
    z = load_golden(name)
    eng = engine_from_fixture(z)
    try:
        eng.set_option("walker", 1)
        th = _rows(z, len(z["thetas"]))
        got = _by_deal(eng, th)
        assert np.isneginf(got[0][1]) and not np.isfinite(got[0][2])
        assert np.isfinite(got[0]).sum() >= 1
        for mode in DEALS[1:]:
            assert np.array_equal(got[mode], got[0], equal_nan=True), (name, mode)
        d = eng.walker_deals(0)
        if d["ntiles"] == 1:
            assert d["deals"] == [[0], [0]]
    finally:
        eng.close()


@pytest.mark.parametrize("W", [2, 3])
def test_small_batches_with_the_shared_deal_forced(W):
    z = load_golden("c0_mgii")
    eng = engine_from_fixture(z)
    try:
        eng.set_option("walker", 1)
        rows = _rows(z, len(z["thetas"]))
        th = np.ascontiguousarray(rows[:W])
        got = _by_deal(eng, th)
        for mode in DEALS[1:]:
            assert np.array_equal(got[mode], got[0], equal_nan=True), (W, mode)
        # row by row the batch's values are those of the fixture's whole batch
        eng.set_option("walker_perm", 2)
        whole = _lnprob_device(eng, rows)
        assert np.array_equal(got[2], whole[:W], equal_nan=True)
    finally:
        eng.close()


def test_stretch_chain_does_not_depend_on_the_deal():
    z = load_golden("c0_mgii")
    fin = np.isfinite(z["lnprob"])
    base = z["thetas"][fin]
    rng = np.random.default_rng(5)
    pos = base[np.arange(64) % len(base)] * (1.0 + 1e-6 * rng.standard_normal((64, base.shape[1])))
    pos = np.ascontiguousarray(np.clip(pos, z["lb"] + 1e-9, z["ub"] - 1e-9))
    chains = {}
    for mode in (0, 2):
        eng = engine_from_fixture(z)
        try:
            eng.set_option("walker", 1)
            eng.set_option("walker_perm", mode)
            p, lp, chain, chain_lp, nacc = eng.stretch_run(pos.copy(), 20, seed=11)
            chains[mode] = (p, lp, chain, chain_lp, np.asarray(nacc))
        finally:
            eng.close()
    assert np.isfinite(chains[0][1]).all() and chains[0][4].sum() > 0
    for a, b in zip(chains[0], chains[2]):
        assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", FIXTURES)
def test_deals_are_permutations_and_entry_waves_hold_the_cheapest_tiles(name):
    z = load_golden(name)
    eng = engine_from_fixture(z)
    try:
        d = eng.walker_deals(0)
        nt, ntask, cost = d["ntiles"], d["ntask"], d["cost"]
        assert 1 <= nt <= 16 and 1 <= ntask <= nt and len(cost) == nt
        for deal in d["deals"]:
            assert sorted(deal) == list(range(nt))
            entry = [cost[t] for t in deal[:ntask]]
            rest = [cost[t] for t in deal[ntask:]]
            assert not rest or max(entry) <= min(rest), (name, deal, cost, ntask)
        shared = d["deals"][1]
        # the grid-order deal: tile order inside the entry waves, inside the line-core tiles behind them, inside the rest
        heavy = [t for t in shared[ntask:] if 2 * cost[t] > max(cost)]
        assert shared[:ntask] == sorted(shared[:ntask])
        assert shared[ntask:ntask + len(heavy)] == sorted(heavy)
        assert shared[ntask + len(heavy):] == sorted(shared[ntask + len(heavy):])
    finally:
        eng.close()
