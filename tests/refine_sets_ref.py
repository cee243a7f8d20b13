"""The cases dvh_lm_normal_sets is held to, shared by tests/test_refine_sets_host.py and tests/test_refine_sets_gpu.py:
observation sets over the random problems of tests/refine_ref.py and the reduced tables that define what an absent
sample means.  Every case is built once (lru_cache) and never modified: the tests copy what they change."""
import functools

import numpy as np

from tests import refine_ref as ref

N_SET = 3
MODEL_SETS = [(2, 0, 2), (1, 1, 0)]  # each a set repeated and a set unused; together they use every set
ABSENT_SHAPE = (3, 8, 13)            # curves of 5, 1 and 7 samples


@functools.lru_cache(maxsize=None)
def present_sets(n_layer, D, S):
    """(set_obs, set_sigma) [N_SET, S]: the case's own observations and two seeded perturbations of them with
    perturbed sigma, every sample present."""
    tab = ref.normal_case(n_layer, D, S)["tab"]
    rng = np.random.default_rng(31 + 1000 * n_layer + 10 * S + D)
    obs = np.stack([tab["sample_obs"]] + [tab["sample_obs"] + rng.normal(0.0, 0.03, S) for _ in range(N_SET - 1)])
    sigma = np.stack([tab["sample_sigma"]] + [tab["sample_sigma"] * rng.uniform(0.5, 2.0, S)
                                              for _ in range(N_SET - 1)])
    for a in (obs, sigma):
        a.setflags(write=False)
    return obs, sigma


def table_of_set(tab, set_obs, set_sigma, k):
    """The case's table with set k's observations and uncertainties: what dvh_lm_normal takes for that set."""
    return {**tab, "sample_obs": np.ascontiguousarray(set_obs[k]), "sample_sigma": np.ascontiguousarray(set_sigma[k])}


def reduced_table(tab, absent):
    """The table without the samples ``absent``: a curve left without a sample goes with its weight, and the curves
    after it are renumbered."""
    keep = np.setdiff1d(np.arange(tab["sample_obs"].size), absent)
    out = {k: np.ascontiguousarray(tab[k][keep]) for k in ref.TABLE_KEYS}
    left = np.unique(out["sample_curve"])
    out["sample_curve"] = np.searchsorted(left, out["sample_curve"]).astype(np.int32)
    out["curve_weight"] = np.ascontiguousarray(tab["curve_weight"][left])
    return out


def absent_cases():
    """(name, absent sample indices) on ABSENT_SHAPE: one sample of the five-sample curve, the whole one-sample curve,
    and both."""
    curve = ref.normal_case(*ABSENT_SHAPE)["tab"]["sample_curve"]
    one = np.flatnonzero(curve == 0)[2:3]
    whole = np.flatnonzero(curve == 1)
    assert one.size == 1 and whole.size == 1
    return [("one sample of a curve", one), ("the whole one-sample curve", whole),
            ("both", np.concatenate([one, whole]))]


def with_absent(set_obs, k, absent):
    """A copy of set_obs with the samples ``absent`` of set k made NaN."""
    out = set_obs.copy()
    out[k, absent] = np.nan
    return out
