"""The random-walk filter on incidence under negative-binomial reports, restated (a helper for
the tests, no test itself): tests/walk_incidence_restatement.py's one_pass with the product weight of
tests/negbin_restatement.py in place of the binomial one for the duration of the call.  Neither file is edited."""
import negbin_restatement as nr
import walk_incidence_restatement as wr


def one_pass(counts, model, theta, hw, probs, kappa, npop, mu, key, f, cumulate=False):
    """walk_incidence_restatement.one_pass under negative-binomial reports; the same dict."""
    with nr.negbin_weights(kappa):
        return wr.one_pass(counts, model, theta, hw, False, probs, npop, mu, key, f, cumulate=cumulate)
