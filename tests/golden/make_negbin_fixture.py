"""Writes tests/golden/negbin_small.npz: the overdispersed case counts of the negative-binomial tests (data only).

Every series is the true flows of incidence_small.npz (make_incidence_fixture.py) reported at mean 0.5 x flow with
gamma-Poisson noise of size 2, i.e. negative-binomial reports of dispersion 2: y ~ Poisson(Gamma(2, 0.5 flow / 2)).
  over          [24, 2]  infections, removals of the SIR epidemic, rng 22
  over_seir     [24, 3]  exposures, onsets, removals of the SEIR epidemic, rng 25
  over_threeday [12, 2]  3-day sums of the first 12 SIR days, reported on days 3, 6, 9, 12 (NaN elsewhere), rng 26
The first values are pinned below: numpy's Generator streams are stable, and a version whose streams differed would
be caught here instead of silently changing what the tests pin.
Run from the repository root:
    python tests/golden/make_negbin_fixture.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RHO, SIZE = 0.5, 2.0


def draw(flows, seed):
    rng = np.random.default_rng(seed)
    return rng.poisson(rng.gamma(SIZE, RHO * flows / SIZE + 1e-300)).astype(np.float64)


def main():
    z = np.load(os.path.join(HERE, "incidence_small.npz"))
    fs, fe = z["sir_flows"], z["seir_flows"]
    over, over_seir = draw(fs, 22), draw(fe, 25)
    sums = fs[:12].reshape(4, 3, -1).sum(axis=1)
    three = np.full((12, 2), np.nan)
    three[2::3] = draw(sums, 26)
    assert over[:, 0].tolist() == [0, 2, 6, 14, 1, 26, 39, 39, 9, 8, 10, 13, 14, 1, 2, 1, 3, 0, 0, 0, 0, 2, 0, 0], over[:, 0]
    assert over[:, 1].tolist() == [0, 3, 7, 2, 2, 1, 0, 22, 4, 1, 36, 10, 1, 10, 4, 5, 7, 2, 2, 4, 1, 1, 3, 4], over[:, 1]
    assert over_seir[:8, 0].tolist() == [1, 3, 6, 0, 2, 6, 10, 11], over_seir[:8, 0]
    assert three[2::3].tolist() == [[2, 10], [46, 8], [79, 27], [62, 14]], three[2::3]
    np.savez(os.path.join(HERE, "negbin_small.npz"), over=over, over_seir=over_seir, over_threeday=three)
    print("wrote negbin_small.npz: over", over.sum(axis=0), "over_seir", over_seir.sum(axis=0))


if __name__ == "__main__":
    main()
