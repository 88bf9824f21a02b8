"""Host side of the G <= 8 subgroup models, no GPU: the new C entry point and ABI version, the Python surface's clear
error above the limit (raised before any context is created), and theta / chain files at 8 groups (65 parameters)."""
import numpy as np
import pytest

from epipf import _lib


def test_max_groups_is_exported_and_eight():
    assert "epipf_max_groups" in _lib.EXPORTS
    assert _lib.load().epipf_max_groups() == 8


def test_abi_version_is_nine():
    assert _lib.ABI_VERSION == 9
    assert _lib.load().epipf_abi_version() == 9


def _forbid_create(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("epipf_create was reached")
    monkeypatch.setattr(_lib.load(), "epipf_create", boom, raising=False)


@pytest.mark.parametrize("model", ["sir_subgroups", "sir_subgroups2"])
def test_nine_groups_raise_value_error_before_any_context(monkeypatch, model):
    from epipf import pmcmc as pm
    from epipf.engine import Engine, get_engine
    from epipf.gillespie import sir_subgroups_simulate
    _forbid_create(monkeypatch)
    G = 9
    msg = r"^subgroup models support at most 8 groups, got 9$"
    beta = np.full((G, G), 1.0)
    Y = np.ones((4, 3 * G if model == "sir_subgroups" else 3))
    npop, mu = np.full(G, 100.0), np.full(G, 5.0)
    with pytest.raises(ValueError, match=msg):
        Engine(model, G, 16, 4, 1)
    with pytest.raises(ValueError, match=msg):
        get_engine(model, G, 16, 4)
    with pytest.raises(ValueError, match=msg):
        pm.particle_filter(Y, model, (beta, 0.5), False, 0.1, 16, npop, mu, key=1, filter_index=0)
    with pytest.raises(ValueError, match=msg):
        pm.particle_mcmc(Y, model, list(beta.reshape(-1)) + [0.5], 0.01, False, None, 2, False, 0.1, 16, npop, mu,
                         progress=False)
    with pytest.raises(ValueError, match=msg):
        sir_subgroups_simulate(np.tile([90.0, 10.0, 0.0], (G, 1)), beta, 0.5, 1.0, True, key=1)


def test_eight_groups_pass_the_check():
    from epipf.engine import check_groups, max_groups
    assert max_groups() == 8
    for mid in (_lib.SIR_SUBGROUPS, _lib.SIR_SUBGROUPS2):
        check_groups(mid, 8)
    check_groups(_lib.SIR, 1)


def test_theta_vector_round_trips_eight_groups():
    from epipf.engine import theta_vector
    beta = np.random.RandomState(3).uniform(0.1, 4.0, (8, 8))
    th, G = theta_vector(_lib.SIR_SUBGROUPS, (beta, 0.7))
    assert G == 8 and th.shape == (65,)
    np.testing.assert_array_equal(th[:64].reshape(8, 8), beta)
    assert th[64] == 0.7


def test_chain_files_with_65_theta_columns(tmp_path):
    from epipf import chains_io
    rs = np.random.RandomState(4)
    thetas = rs.uniform(0.1, 3.0, (40, 65))
    thetas[10:20] = thetas[10]                           # rejected proposals repeat the row
    lik = rs.uniform(0.0, 1.0, 40)
    trajs = rs.randint(0, 300, (5, 40, 24)).astype(float)
    chains_io.save_run(str(tmp_path), thetas, lik, trajs)
    t2, l2, tr2 = chains_io.load_run(str(tmp_path), C=24)
    np.testing.assert_array_equal(t2, thetas)
    np.testing.assert_array_equal(l2, lik)
    np.testing.assert_array_equal(tr2, trajs)
    start, sigma = chains_io.warm_start(t2, burn_in=5, thin=3)
    assert len(start) == 65 and start == thetas[-1].tolist()
    assert sigma.shape == (65, 65)
    np.testing.assert_allclose(sigma, sigma.T)
