"""The numpy restatement of iterated filtering for the subgroup models (tests/if2_sub_restatement.py)
against the CPU oracle, and what every input of the GPU tests (tests/if2_sub_cases.py) contains: which searches
complete, which degenerate and where, reflections and event counts.  No GPU."""
import numpy as np
import pytest

import if2_restatement as rs
import if2_sub_cases as sc
import if2_sub_restatement as srs
import oracle


@pytest.fixture(scope="module")
def fx():
    return sc.load_fixture()


def test_theta_layout_round_trips():
    beta, gamma = srs.to_pair(np.arange(10.0))
    np.testing.assert_array_equal(beta, np.arange(9.0).reshape(3, 3))
    assert gamma == 9.0 and srs.groups_of(17) == 4
    np.testing.assert_array_equal(srs.to_flat(beta, gamma), np.arange(10.0))
    np.testing.assert_array_equal(sc.rw_of(2), [0.1, 0.05, 0.05, 0.1, 0.05])


def test_draws_of_the_last_block(fx):
    """d = 5 and 17 use the first half of their last block, d = 10 all of it; the columns shared with a shorter theta are
    the same draws."""
    u17 = rs.perturb_uniforms(9, 2, 3, 7, 17)
    for d in (5, 10):
        np.testing.assert_array_equal(rs.perturb_uniforms(9, 2, 3, 7, d), u17[:, :d])
    assert len(np.unique(u17)) == u17.size


def test_group_sums(fx):
    x = np.arange(12).reshape(2, 6)
    np.testing.assert_array_equal(srs.observed("sir_subgroups2", x), [[3, 5, 7], [15, 17, 19]])
    assert srs.observed("sir_subgroups", x) is x
    assert fx[3]["sir_subgroups2"].shape == (20, 3) and fx[3]["sir_subgroups"].shape == (20, 9)


@pytest.mark.parametrize("G", sc.GROUPS)
@pytest.mark.parametrize("observations", [False, True])
@pytest.mark.parametrize("model", sc.MODELS)
def test_no_jitter_is_the_oracle_filter(fx, model, observations, G):
    """Zero half-widths and equal theta: one pass is oracle.particle_filter bit for bit."""
    c = sc.case(fx, model, G, 40, 8, M=1, observations=observations, hw=np.zeros((1, G * G + 1)))
    r = sc.restate(c)
    o = oracle.particle_filter(c["Y"], model, srs.to_pair(fx[G]["theta"]), observations, c["probs"], 40, c["npop"],
                               c["mu"], key=c["key"], filter_index=c["f"])
    assert r["status"] == o["status"] == 0 and r["iterations_done"] == 1 and r["reflections"] == 0
    np.testing.assert_array_equal(r["swarm"], c["swarm0"])
    np.testing.assert_array_equal(r["hidden"], o["hidden"])
    np.testing.assert_array_equal(r["ancestry"], o["ancestry"])
    np.testing.assert_array_equal(r["log_zetas"][0], o["log_zetas"])
    assert r["events"][0] == o["events"]


# ------------------------------------------------------------------------------------------- the GPU tests' inputs
PARITY_EVENTS = {("sir_subgroups", 2): [18108, 19613, 19146], ("sir_subgroups", 3): [19764, 19172, 20016],
                 ("sir_subgroups", 4): [14673, 15197, 16705], ("sir_subgroups2", 2): [19687, 19087, 19121],
                 ("sir_subgroups2", 3): [18733, 18889, 19386], ("sir_subgroups2", 4): [12695, 11791, 11410]}


@pytest.mark.parametrize("G", sc.GROUPS)
@pytest.mark.parametrize("model", sc.MODELS)
def test_parity_cases_complete_every_iteration(fx, model, G):
    r = sc.restate(sc.parity_case(fx, model, G))
    assert r["status"] == 0 and r["iterations_done"] == 3 and np.isfinite(r["log_zetas"]).all()
    assert sc.distinct(r["swarm"]) == 65 and r["events"].tolist() == PARITY_EVENTS[model, G]


def test_reflection_case_reflects(fx):
    r = sc.restate(sc.reflection_case(fx))
    assert r["status"] == 0 and r["iterations_done"] == 2
    assert r["reflections"] == 334 and (r["swarm"] >= 0.0).all() and r["events"].tolist() == [97, 212]


@pytest.mark.parametrize("model,events", [("sir_subgroups", [10441, 10586]), ("sir_subgroups2", [9387, 9208])])
def test_fixed_components_stay_fixed(fx, model, events):
    c = sc.fixed_case(fx, model)
    r = sc.restate(c)
    assert r["status"] == 0 and r["iterations_done"] == 2 and r["events"].tolist() == events
    off = r["swarm"][:, 1:3]
    assert set(np.unique(off)) == {0.0, 0.3} and (off[:, 0] == off[:, 1]).all()      # both kinds survive, rows intact
    assert sc.distinct(r["swarm"]) == 130
    assert {tuple(v) for v in c["swarm0"][:64, 1:3]} == {(0.0, 0.0), (0.3, 0.3)}   # both kinds in the first wave


BATCH_EVENTS = [[18332, 18895, 18372], [20246, 20082, 20562], [19279, 19317, 18710]]


def test_batch_cases_complete(fx):
    for M in (2, 3):
        for s, c in enumerate(sc.batch_cases(fx, M)):
            r = sc.restate(c)
            assert r["status"] == 0 and r["iterations_done"] == M and r["events"].tolist() == BATCH_EVENTS[s][:M]
    assert (int(sc.F0[2]) + 1) & 0xFFFFFFFF == 0


def test_degenerate_case_dies_at_once_between_two_that_complete(fx):
    rs_ = [sc.restate(c) for c in sc.degenerate_cases(fx)]
    assert [r["status"] for r in rs_] == [0, 1, 0] and [r["iterations_done"] for r in rs_] == [3, 0, 3]
    assert int(np.argmax(np.isneginf(rs_[1]["last_log_zetas"]))) == 2
    np.testing.assert_array_equal(rs_[1]["swarm"], sc.degenerate_cases(fx)[1]["swarm0"])
    assert [r["events"].tolist() for r in rs_] == [[20077, 20293, 22336], [9751, 0, 0], [21756, 20484, 21646]]


PATH_EVENTS = {("sir_subgroups", 2): [11618, 11162], ("sir_subgroups", 3): [15229, 16495],
               ("sir_subgroups", 4): [14869, 14528], ("sir_subgroups2", 2): [10840, 11407],
               ("sir_subgroups2", 3): [14223, 15765], ("sir_subgroups2", 4): [12274, 12463]}


@pytest.mark.parametrize("G", sc.GROUPS)
@pytest.mark.parametrize("model", sc.MODELS)
def test_path_cases_complete(fx, model, G):
    r = sc.restate(sc.path_case(fx, model, G))
    assert r["status"] == 0 and r["iterations_done"] == 2 and r["events"].tolist() == PATH_EVENTS[model, G]
    assert sc.distinct(r["swarm"]) == 130


@pytest.mark.parametrize("model", sc.MODELS)
def test_the_searches_of_the_end_to_end_test(fx, model):
    """Both searches complete all 12 iterations and gain what tests/if2_sub_cases.py records (the GPU test asserts half
    the smaller gain): sir_subgroups 25.74 and 14.91, sir_subgroups2 35.38 and 30.67 log units over the start."""
    g = fx[2]
    start = srs.score(g[model], model, np.array(sc.SEARCH["start"]), False, fx["probs"], g["npop"], g["mu"])
    assert start == pytest.approx(sc.START_SCORE[model], rel=1e-12)
    for s in range(sc.SEARCHES):
        r = sc.restate(sc.search_case(fx, model, s))
        assert r["status"] == 0 and r["iterations_done"] == sc.SEARCH["M"]
        final = srs.score(g[model], model, r["mean"][-1], False, fx["probs"], g["npop"], g["mu"])
        assert final == pytest.approx(sc.FINAL_SCORE[model][s], rel=1e-12)
    assert min(sc.cpu_gains(model)) > 14.0


def test_the_third_search_would_degenerate(fx):
    r = sc.restate(sc.search_case(fx, "sir_subgroups", 2))
    assert (r["status"], r["iterations_done"]) == (1, 2)
