"""Time-varying rates on the CPU: the random-walk filter's restatement (tests/walk_restatement.py) against
§17's one_pass, epipf.walk's numpy backend against a brute-force reduction, the reduction's properties bit for bit, and
the "does it work" numbers on the step fixture."""
import numpy as np
import pytest

import if2_restatement as rs
import walk_cases as wc
import walk_restatement as wr
from epipf import walk

THETA = {"sir": (0.8, 0.3), "seir": (0.9, 0.6, 0.3)}
RW = {"sir": (0.1, 0.05), "seir": (0.1, 0.08, 0.05)}
PROBS = {False: 0.5, True: 0.2}


def if2_fixture():
    import if2_cases
    return if2_cases.load_fixture()


# ------------------------------------------------------------------------------------------- the pass
@pytest.mark.parametrize("observations", [False, True])
@pytest.mark.parametrize("model", ["sir", "seir"])
def test_the_pass_is_section_17s(model, observations):
    fx = if2_fixture()
    N, T = 24, 9
    swarm = np.tile(np.array(THETA[model]), (N, 1))
    args = (fx[model][:T], model, swarm, RW[model], observations, PROBS[observations], fx["npop"], fx["mu"], 11, 3)
    want, got = rs.one_pass(*args), wr.one_pass(*args)
    assert got["status"] == want["status"] == 0
    np.testing.assert_array_equal(got["hidden"], want["hidden"])
    np.testing.assert_array_equal(got["ancestry"], want["ancestry"])
    np.testing.assert_array_equal(wr.bits(got["log_zetas"]), wr.bits(want["log_zetas"]))
    np.testing.assert_array_equal(wr.bits(got["theta_hist"][T - 1]), wr.bits(want["theta"]))
    assert len(np.unique(got["theta_hist"][T - 1], axis=0)) > 1


def test_a_dying_pass_keeps_its_earlier_rows():
    fx = if2_fixture()
    args = (fx["sir"], "sir", np.tile((2.0, 1.0), (48, 1)), (0.1, 0.05), False, fx["probs"], fx["npop"], fx["mu"], 2, 0)
    want, got = rs.one_pass(*args), wr.one_pass(*args)
    assert got["status"] == want["status"] == wr.DEGENERATE
    dead = int(np.argmax(np.isneginf(got["log_zetas"])))
    assert dead >= 1 and np.isneginf(got["log_zetas"][dead:]).all()
    np.testing.assert_array_equal(got["log_zetas"], want["log_zetas"])
    assert np.isfinite(got["theta_hist"][:dead]).all() and np.isnan(got["theta_hist"][dead:]).all()


# ------------------------------------------------------------------------------------------- the numpy backend
def check_backend(hid, anc, th, pop, lineage, lag, q):
    mean, qs, lin = walk.smooth_history(hid, anc, th, pop, lag=lag, quantiles=q, lineage=lineage)
    bmean, bqs, blin = wr.brute_force(hid, anc, th, pop, 1 if lineage == "genealogy" else 0, lag, q)
    np.testing.assert_array_equal(lin, blin)
    wr.assert_mean_close(mean, bmean, anc.shape[1])
    if q is None:
        assert qs is None
    else:
        np.testing.assert_array_equal(wr.bits(qs), wr.bits(bqs))
    return mean, qs, lin


@pytest.mark.parametrize("lineage", ["genealogy", "reference"])
def test_backend_on_the_golden_histories(filter_golden, lineage):
    """The filter goldens' histories with a synthetic theta attached."""
    done = 0
    for name, rec in sorted(filter_golden.items()):
        if "hidden" not in rec or rec["hidden"].shape[2] > 4 or int(rec["status"]) != 0 or done >= 4:
            continue
        hid, anc = rec["hidden"].astype(np.int32), rec["ancestry"].astype(np.int32)
        T, N, C = hid.shape
        rng = np.random.default_rng(T * 1000 + N)
        th = np.abs(rng.normal(0.6, 0.3, size=(T, N, 2)))
        for lag in (0, 1, 3, None):
            check_backend(hid, anc, th, float(hid[0, 0].sum()), lineage, lag, (0.05, 0.5, 0.95))
        done += 1
    assert done >= 2


@pytest.mark.parametrize("shape", [(1, 1, 3, 2), (2, 5, 4, 3), (7, 65, 3, 2), (7, 64, 4, 3)])
def test_backend_on_the_hand_made_histories(shape):
    T, N, C, d = shape
    hid, anc, th, names = wc.chains(T, N, C, d, seed=T + N)
    for k, name in enumerate(names):
        for li, lineage in enumerate(("genealogy", "reference")):
            for L in wc.lags(T)[(k + li) % 2::2]:
                check_backend(hid[k], anc[k], th[k], 300.0, lineage, L, wc.QUANTILES)


# ------------------------------------------------------------------------------------------- properties, bit for bit
@pytest.fixture(scope="module")
def a_history():
    r = wc.restated(1, True)
    return r["hidden"], r["ancestry"], r["theta_hist"]


@pytest.mark.parametrize("lineage", ["genealogy", "reference"])
def test_properties(a_history, lineage):
    hid, anc, th = a_history
    T, N = anc.shape
    kw = dict(quantiles=(0.05, 0.5, 0.95), lineage=lineage)
    cloud = walk.smooth_history(hid, anc, th, 300.0, lag=0, **kw)
    assert (cloud[2] == N).all()                         # L = 0 is the particle cloud
    full = walk.smooth_history(hid, anc, th, 300.0, lag=None, **kw)
    for L in (T - 1, T, 10 ** 6):                        # L >= T-1 is the full smoother
        got = walk.smooth_history(hid, anc, th, 300.0, lag=L, **kw)
        for a, b in zip(got, full):
            np.testing.assert_array_equal(wr.bits(a) if a.dtype == np.float64 else a, wr.bits(b) if b.dtype == np.float64 else b)
    last = cloud[2]
    for L in range(1, T):                                # lineages do not increase with L
        lin = walk.smooth_history(hid, anc, th, 300.0, lag=L, **kw)[2]
        assert (lin <= last).all()
        last = lin
    const = th.copy()
    const[:, :, 1] = 0.2                                 # a column constant over the particles: that constant everywhere
    _, qs, _ = walk.smooth_history(hid, anc, const, 300.0, lag=5, quantiles=wc.QUANTILES, lineage=lineage)
    assert (wr.bits(qs[:, :, 1]) == wr.bits(np.float64(0.2))).all()


def test_smooth_history_refuses_bad_input(a_history):
    hid, anc, th = a_history
    bad = th.copy()
    for v in (-1.0, np.nan, np.inf):
        bad[3, 4, 0] = v
        with pytest.raises(ValueError):
            walk.smooth_history(hid, anc, bad, 300.0)
    with pytest.raises(ValueError):
        walk.smooth_history(hid, anc[:, :-1], th, 300.0)
    with pytest.raises(ValueError):
        walk.smooth_history(hid, anc, th, 300.0, lag=-1)
    with pytest.raises(ValueError):
        walk.smooth_history(hid, anc, th, 300.0, lineage="tree")
    with pytest.raises(ValueError):
        walk.smooth_history(hid, anc, th, 300.0, quantiles=(1.5,))
    with pytest.raises(ValueError):
        walk.smooth_history(hid, anc, th, 0.0)


# ------------------------------------------------------------------------------------------- does it work
def test_the_walk_finds_the_step_and_the_likelihood_prefers_it():
    """Per key 1..4: the smoothed median of beta (lag 5) falls from the early to the late plateau by at least GAP_BOUND,
    and the random-walk model's log-likelihood exceeds the constant-rate one's by at least GAIN_BOUND; both are half the
    smallest value measured over the four keys (walk_cases.py has the table)."""
    gaps, gains = [], []
    for key in wc.KEYS:
        r, r0 = wc.restated(key, True), wc.restated(key, False)
        assert r["status"] == 0 and r0["status"] == 0
        _, qs, _ = walk.smooth_history(r["hidden"], r["ancestry"], r["theta_hist"], 300.0, lag=wc.LAG_WORK, quantiles=(0.5,))
        gaps.append(wc.plateau_gap(qs[0, :, 0]))
        gains.append(r["log_zetas"][-1] - r0["log_zetas"][-1])
        assert (wr.bits(r["theta_hist"][:, :, 1]) == wr.bits(np.float64(0.2))).all()   # rw = 0 keeps gamma bit for bit
    print("gaps", gaps, "gains", gains)
    assert min(gaps) > wc.GAP_BOUND and min(gains) > wc.GAIN_BOUND
