"""The CPU oracle at G = 5, 6 and 8 groups against the unmodified reference's output
(tests/golden/wide_groups_golden.npz, written by tests/golden/make_golden_wide.py under the keyed-stream shim):
states and ancestors bit for bit, log-likelihoods within 1e-12."""
import numpy as np
import pytest

import oracle
from conftest import case_args, load_golden

CASES = ["wide_sir_subgroups_g6", "wide_sir_subgroups2_g5", "wide_sir_subgroups_g8"]


@pytest.mark.parametrize("case", CASES)
def test_oracle_equals_reference_above_four_groups(case):
    rec = load_golden("wide_groups_golden.npz")[case]
    a = case_args(rec)
    assert a["theta"][0].shape[0] == {"g6": 6, "g5": 5, "g8": 8}[case[-2:]]
    o = oracle.particle_filter(a["Y"], a["model"], a["theta"], a["observations"], a["probs"], a["N"], a["npop"],
                               a["mu"], key=a["key"], filter_index=a["f"])
    assert o["status"] == int(rec["status"]) == 0
    np.testing.assert_array_equal(o["hidden"], rec["hidden"])
    np.testing.assert_array_equal(o["ancestry"], rec["ancestry"])
    np.testing.assert_allclose(o["log_zetas"], np.log(rec["zetas"]), rtol=0, atol=1e-12)
