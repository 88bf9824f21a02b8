"""epipf.if2_subgroups' host logic over an oracle-backed engine double (tests/if2_sub_oracle_engine.py): both forms of
`start` and `rw`, fixed components, .beta / .gamma, continue_, evaluate and best, and the ValueErrors raised before any
engine exists.  No GPU."""
import importlib

import numpy as np
import pytest

import if2_sub_cases as sc
import if2_sub_oracle_engine
import if2_sub_restatement as srs

mod = importlib.import_module("epipf.if2")               # epipf.if2 itself is the function

START = [1.0, 0.2, 0.4, 1.1, 0.4]
RW = [0.1, 0.05, 0.05, 0.1, 0.05]


@pytest.fixture()
def engines(monkeypatch):
    made = []

    def get(*a, **k):
        made.append(if2_sub_oracle_engine.fake_get_engine(*a, **k))
        return made[-1]
    monkeypatch.setattr(mod._engine, "get_engine", get)
    return made


@pytest.fixture(scope="module")
def data():
    fx = sc.load_fixture()
    return dict(fx=fx, Y=fx[2]["sir_subgroups"][:8], n_population=fx[2]["npop"], mu=fx[2]["mu"], probs=fx["probs"])


def call(data, start, rw=RW, model="sir_subgroups", **kw):
    import epipf
    epipf.seed_stream(21, 5)
    args = dict(iterations=3, cooling=0.5, n_particles=16, searches=1, evaluate=False, n_population=data["n_population"],
                mu=data["mu"], probs=data["probs"])
    args.update(kw)
    return epipf.if2_subgroups(args.pop("Y", data["Y"]), model, start, rw, **args)


def test_the_call_the_engine_sees(data, engines):
    res = call(data, START, searches=2)
    (eng,) = engines
    assert (eng.mid, eng.G, eng.max_chains, eng.N) == (2, 2, 2, 16) and not eng.run_calls
    (c,) = eng.if2_calls
    np.testing.assert_array_equal(c["swarm"], np.tile(START, (2, 16, 1)))
    np.testing.assert_array_equal(c["hw"], mod.cooling_table(RW, 0.5, 3))
    assert c["keys"].tolist() == [21, 21 + (1 << 32)] and c["f0"].tolist() == [5, 5]
    assert mod._STREAM.next_filter == 8
    assert res.theta.shape == (2, 5) and res.trace.shape == (2, 3, 5) and res.loglik.shape == (2, 3)
    assert res.swarm.shape == (2, 16, 5) and res.loglik_at_theta is None and res.best is None
    np.testing.assert_array_equal(res.theta, res.trace[:, -1])
    assert (res.status == 0).all() and (res.iterations_done == 3).all()
    r = srs.run(data["Y"], "sir_subgroups", np.tile(START, (16, 1)), c["hw"], False, data["probs"], data["n_population"],
                data["mu"], 21, 5)
    np.testing.assert_array_equal(res.swarm[0], r["swarm"])


def test_beta_and_gamma_are_views_of_theta(data, engines):
    res = call(data, START, searches=2, iterations=1)
    assert res.beta.shape == (2, 2, 2) and res.gamma.shape == (2,)
    np.testing.assert_array_equal(res.beta.reshape(2, 4), res.theta[:, :4])
    np.testing.assert_array_equal(res.gamma, res.theta[:, 4])
    assert np.shares_memory(res.beta, res.theta) and np.shares_memory(res.gamma, res.theta)
    assert len(list(res.theta[0])) == 5                  # particle_mcmc's flat params


def test_the_reference_form_of_start_and_rw_equals_the_flat_one(data, engines):
    beta, gamma = srs.to_pair(np.array(START))
    rbeta, rgamma = srs.to_pair(np.array(RW))
    flat = call(data, START, iterations=1)
    pair = call(data, (beta, gamma), (rbeta, rgamma), iterations=1)
    mixed = call(data, (beta.tolist(), gamma), RW, iterations=1)
    for eng in engines[1:]:
        np.testing.assert_array_equal(eng.if2_calls[0]["swarm"], engines[0].if2_calls[0]["swarm"])
        np.testing.assert_array_equal(eng.if2_calls[0]["hw"], engines[0].if2_calls[0]["hw"])
    np.testing.assert_array_equal(pair.swarm, flat.swarm)
    np.testing.assert_array_equal(mixed.swarm, flat.swarm)


def test_start_per_search_in_both_forms(data, engines):
    other = [1.2, 0.3, 0.3, 0.9, 0.35]
    call(data, [START, other], searches=2, iterations=1)
    call(data, [srs.to_pair(np.array(START)), srs.to_pair(np.array(other))], searches=2, iterations=1)
    for eng in engines:
        sw = eng.if2_calls[0]["swarm"]
        np.testing.assert_array_equal(sw[0], np.tile(START, (16, 1)))
        np.testing.assert_array_equal(sw[1], np.tile(other, (16, 1)))


def test_a_zero_rw_fixes_the_component(data, engines):
    start = [1.0, 0.0, 0.0, 1.1, 0.4]
    res = call(data, start, [0.1, 0.0, 0.0, 0.1, 0.05])
    assert (res.swarm[0][:, 1:3] == 0.0).all() and (res.beta[0][[0, 1], [1, 0]] == 0.0).all()
    assert sc.distinct(res.swarm[0]) > 1
    np.testing.assert_array_equal(engines[0].if2_calls[0]["hw"][:, 1:3], np.zeros((3, 2)))


def test_three_groups_from_flat_input_take_G_from_mu(data, engines):
    fx = data["fx"]
    res = call(data, fx[3]["theta"], sc.rw_of(3), model="sir_subgroups2", Y=fx[3]["sir_subgroups2"][:6],
               n_population=fx[3]["npop"], mu=fx[3]["mu"], iterations=1)
    assert engines[0].G == 3 and engines[0].mid == 3 and res.beta.shape == (1, 3, 3)


def test_continue_equals_one_longer_run(data, engines):
    whole = call(data, START, iterations=3)
    part = call(data, START, iterations=1)
    more = part.continue_(2)
    c = engines[1].if2_calls
    assert len(c) == 2 and c[1]["f0"].tolist() == [6]
    np.testing.assert_array_equal(c[1]["swarm"], part.swarm)
    np.testing.assert_array_equal(c[1]["hw"], mod.cooling_table(RW, 0.5, 2, first=1))
    np.testing.assert_array_equal(more.swarm, whole.swarm)
    np.testing.assert_array_equal(more.trace, whole.trace)
    np.testing.assert_array_equal(more.loglik, whole.loglik)
    assert more.iterations_done.tolist() == [3] and mod._STREAM.next_filter == 8 and more.beta.shape == (1, 2, 2)


def test_evaluate_scores_theta_with_plain_filters_and_picks_the_best(data, engines):
    res = call(data, [START, [3.0, 1.5, 1.5, 3.0, 0.2]], searches=2, evaluate=True)
    (eng,) = engines
    assert eng.max_chains == 16
    (r,) = eng.run_calls                                 # one batched run: 8 filters per search
    np.testing.assert_array_equal(r["thetas"], np.repeat(res.theta, 8, axis=0))
    assert r["fidx"].tolist() == list(range(8)) * 2
    assert r["keys"].tolist() == [21 + (2 << 32)] * 8 + [21 + (3 << 32)] * 8       # keys no search uses
    for s in range(2):
        want = srs.score(data["Y"], "sir_subgroups", res.theta[s], False, data["probs"], data["n_population"],
                         data["mu"], n_particles=16, key=int(r["keys"][8 * s]))
        assert res.loglik_at_theta[s] == pytest.approx(want, rel=1e-12)
    assert res.best == int(np.argmax(res.loglik_at_theta))


def test_value_errors_come_before_any_engine(data, engines):
    import epipf
    big = np.full(26, 0.5)
    with pytest.raises(ValueError, match="G <= 4"):      # G = 5 from mu
        call(data, big, np.full(26, 0.01), Y=np.zeros((4, 15)), n_population=[50] * 5, mu=[2] * 5)
    with pytest.raises(ValueError, match="G <= 4"):      # G = 5 from beta
        call(data, (np.full((5, 5), 0.5), 0.3), np.full(26, 0.01), Y=np.zeros((4, 15)), n_population=[50] * 5, mu=[2] * 5)
    with pytest.raises(ValueError):                      # one group
        call(data, [1.0, 0.3], [0.1, 0.05], Y=np.zeros((4, 3)), n_population=[50], mu=[2])
    for start, rw in ((START[:4], RW), (START, RW[:4]), ([START] * 3, RW), ([-1.0] + START[1:], RW),
                      (START, [-0.1] + RW[1:]), ((np.ones((2, 3)), 0.3), RW), ((np.ones((3, 3)), 0.3), RW)):
        with pytest.raises(ValueError):
            call(data, start, rw, searches=2)
    with pytest.raises(ValueError):                      # Y's columns against G
        call(data, START, Y=np.zeros((4, 9)))
    with pytest.raises(ValueError):                      # the population against G
        call(data, START, n_population=[100, 100, 100])
    with pytest.raises(ValueError):
        call(data, START, iterations=0)
    for model in ("sir", epipf.ModelType.SEIR):
        with pytest.raises(ValueError, match=r"epipf\.if2 "):
            epipf.if2_subgroups(data["Y"], model, (1.0, 0.4), (0.1, 0.05))
    assert not engines


def test_if2_points_to_the_new_entry_point(data, engines):
    import epipf
    with pytest.raises(ValueError, match="if2_subgroups"):
        epipf.if2(data["Y"], "sir_subgroups", (1.0, 0.4), (0.1, 0.05))
    assert not engines and "if2_subgroups" in epipf.__all__
