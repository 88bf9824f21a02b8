"""The phases the one-lane step kernels share (csrc/epipf_step.hpp), compared across the kernels that
call them: the plain filter's step kernel, IF2's and the random-walk filter's at zero half-widths run the same
particles, so their histories, log-likelihood bits and device counters must agree (case A); and the incidence filter's
event counter, with every lane on the exact SSA loop, against the plain filter's over the rows both filters share and
against the events its own history shows (case B).  Needs an MI355X."""
import numpy as np
import pytest

import if2_cases
import incidence_cases as ic

pytestmark = pytest.mark.gpu

KEY, F = if2_cases.KEY, if2_cases.F
COUNTERS = 2                                             # EPIPF_PROFILE_COUNTERS


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


@pytest.fixture(scope="module")
def fx():
    return if2_cases.load_fixture()


def step_engine(monkeypatch, model, N, T):
    """An engine whose filters take the one-lane step launches, with the device counters on."""
    from epipf.engine import Engine
    monkeypatch.setenv("EPIPF_FUSED", "0")
    eng = Engine(model, 1, N, T, 1)
    eng.set_lanes(1)
    eng.set_profiling(COUNTERS)
    return eng


def counters(eng, ordered=True):
    """The last run's device counters; ordered: every event took a lane-iteration and every lane-iteration a slot of its
    wave's (not so where the filter replays its lanes cooperatively: the replay counts events but no iterations)."""
    s = eng.stats()
    if ordered:
        assert s["wave_lane_slots"] >= s["lane_iterations"] >= s["events"] >= 0, s
    return s


def dying_step(lz):
    dead = np.isneginf(lz)
    return int(np.argmax(dead)) if dead.any() else None


# ------------------------------------------------------------------------------- A. the variants against the filter
# N = 1: one particle; 65, 130: a partial last block, more than one block; 12,864 = 201 blocks: the first segmented size
@pytest.mark.parametrize("model,N,T", [("sir", 1, 6), ("sir", 65, 6), ("sir", 130, 6), ("seir", 65, 6),
                                       ("sir", 12864, 3)])
def test_if2_and_walk_at_zero_width_are_the_plain_filter(fx, monkeypatch, model, N, T):
    theta = if2_cases.THETA[model]
    d = len(theta)
    eng = step_engine(monkeypatch, model, N, T)
    eng.set_observations(fx[model][:T])
    eng.set_population(fx["npop"], fx["mu"])
    swarm0 = np.tile(np.array(theta), (1, N, 1))
    zero = np.zeros((1, d))

    lz, st = eng.run(np.array([theta]), fx["probs"], KEY, F)
    hid, anc = eng.history(1)
    plain = counters(eng)
    assert plain["last_lanes"] == 1 and plain["last_fused"] == 0

    swarm, _, ilz, done, ist = eng.if2(swarm0, zero, fx["probs"], KEY, F)
    ihid, ianc = eng.history(1)
    if2 = counters(eng)

    wlz, wst = eng.walk_filter(swarm0, zero, fx["probs"], KEY, F)
    whid, wanc = eng.history(1)
    walk = counters(eng)
    eng.close()

    assert st[0] == ist[0] == wst[0]
    rows = T
    if st[0] == 0:
        assert done[0] == 1
        np.testing.assert_array_equal(bits(ilz[0, 0]), bits(lz[0]))
        np.testing.assert_array_equal(bits(swarm), bits(swarm0))         # a zero half-width moves nothing
    else:                                                # all three die at the same step; the rows before it agree
        rows = dying_step(lz[0])
        assert rows is not None and rows >= 1 and rows == dying_step(wlz[0])
    np.testing.assert_array_equal(bits(wlz[0]), bits(lz[0]))
    for h, a in ((ihid, ianc), (whid, wanc)):
        np.testing.assert_array_equal(h[0, :rows], hid[0, :rows])
        np.testing.assert_array_equal(a[0, :rows], anc[0, :rows])
    # lane_iterations is not compared: the filter's cooperative replay counts them differently from the per-lane exact
    # loop of the variants
    for other in (if2, walk):
        assert other["events"] == plain["events"]
        assert other["resample_fallbacks"] == plain["resample_fallbacks"]
    if st[0] == 0:
        assert plain["events"] > 0


# ------------------------------------------------------------------------------- B. widened bands
def sir_events(hid, anc, first, last):
    """Events of steps first..last of a SIR history [T, N, 3], [T, N]: every event moves one individual out of S or into
    R, so a particle's count over a step is (S' - S) + (R - R') against its parent."""
    n = 0
    for p in range(first, last + 1):
        parent = hid[p - 1][anc[p]]
        n += int((parent[:, 0] - hid[p][:, 0]).sum() + (hid[p][:, 2] - parent[:, 2]).sum())
    return n


def infectious_parents(hid, anc):
    """Particle-steps of a SIR history whose parent has I > 0.  With I = 0 every rate is 0: the lane draws nothing and
    meets no band, so it cannot leave the f32 loop; every other lane draws at least its first clock and, with the bands
    widened, is handed to the exact path."""
    return sum(int((hid[p - 1][anc[p]][:, 1] > 0).sum()) for p in range(1, hid.shape[0]))


def test_incidence_events_on_the_exact_path_against_the_plain_filter(monkeypatch):
    """The incidence oracle (tests/incidence_restatement.py) exposes no event count, so the counter is held against the
    plain filter's for the same theta, key and filter index.  Row 0 weighs 1 in the incidence filter and, with Y = 0 and
    probs = 0, in the plain filter, so both resample row 1 alike: rows 0 and 1 are equal, which is asserted first, and
    the counters are compared over step 1 alone -- each filter's events of the later steps, which its own history
    shows, taken off its total."""
    N, D = 65, 3
    T = D + 2
    monkeypatch.setenv("EPIPF_BAND_SLACK", "3000")       # every channel decision unsure and every clock band hit:
    monkeypatch.setenv("EPIPF_CLOCK_SLACK", "1e10")      # the lanes leave the f32 loop for the exact one
    eng = step_engine(monkeypatch, "sir", N, T)
    eng.set_population(ic.NPOP, ic.MU)
    th = np.array([ic.THETA["sir"]])

    eng.set_observations(np.zeros((T, 3)))
    _, pst = eng.run(th, 0.0, ic.KEY, ic.F)
    phid, panc = eng.history(1)
    plain = counters(eng, ordered=False)                 # its exact path is the cooperative replay

    counts = ic.daily("sir", False, (0, 1), days=D)
    assert np.isfinite(counts).all()                     # every column reported, not cumulated
    _, st = eng.run_incidence(th, 0.5, ic.KEY, ic.F, counts)
    hid, anc = eng.history(1)
    inc = counters(eng)
    eng.close()

    assert pst[0] == 0 and st[0] == 0
    np.testing.assert_array_equal(hid[0, :2], phid[0, :2])
    np.testing.assert_array_equal(anc[0, :2], panc[0, :2])
    # the premise: every lane that can have an event took the exact path
    assert inc["ssa_exact_lanes"] == infectious_parents(hid[0], anc[0]) > 0, inc
    assert plain["ssa_exact_lanes"] == infectious_parents(phid[0], panc[0]) > 0, plain
    step1 = sir_events(hid[0], anc[0], 1, 1)
    assert inc["events"] - sir_events(hid[0], anc[0], 2, T - 1) == step1
    assert plain["events"] - sir_events(phid[0], panc[0], 2, T - 1) == step1
