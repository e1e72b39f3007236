"""tsgo_sample_marginals without a GPU: the generator (known answers, the host entry point tsgo_sample_noise against the Python
restatement) and the restatement itself (tests/posterior.py): its H against the dense oracle's, and the two statistical bounds of
tests/test_gpu_sample_marginals.py at the seeds those tests use — which makes them conditions the reference meets."""
import ctypes as C
import functools

import numpy as np

from oracle import oracle
from tests import lm_rules, posterior, util
from toyslam_amd import _lib

NOISE = _lib.host_lib().tsgo_sample_noise      # (the restatement below qualifies a product that has the generator)


def test_philox_known_answers():
    for counter, key, want in posterior.KNOWN_ANSWERS:
        assert posterior.philox(counter, key) == want
    # ... and the vectorised form is the same function: key = seed, counter = (index, tag, k, 0)
    w = posterior.philox_words((0x299f31d0 << 32) | 0xa4093822, 0x85a308d3, np.array([0x243f6a88]), np.array([0x13198a2e]))[0]
    assert tuple(int(x) for x in w) == posterior.philox((0x243f6a88, 0x85a308d3, 0x13198a2e, 0), (0xa4093822, 0x299f31d0))


def test_host_noise_is_the_restatement():
    rng = np.random.default_rng(5)
    n = 1000
    seeds = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    tags = rng.integers(0, 2, n); index = rng.integers(0, 2 ** 32, n, dtype=np.uint64); k = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    index[:4] = [0, 2 ** 32 - 1, 0, 2 ** 32 - 1]; k[:4] = [0, 0, 2 ** 32 - 1, 2 ** 32 - 1]
    words = (C.c_uint32 * 4)(); nrm = (C.c_double * 4)()
    worst = 0.0
    for j in range(n):
        NOISE(int(seeds[j]), int(tags[j]), int(index[j]), int(k[j]), words, nrm)
        want = posterior.philox((int(index[j]), int(tags[j]), int(k[j]), 0), (int(seeds[j]) & posterior.MASK, int(seeds[j]) >> 32))
        assert tuple(words) == want, j
        ref = posterior.box_muller(np.array(want, np.uint64))
        assert np.abs(ref).max() <= 7.0
        worst = max(worst, float(np.abs(np.array(nrm) - ref).max()))
    assert worst <= 1e-12, worst      # a few ulp of values <= 7: two libms may differ in the last place
    NOISE(1, 0, 2, 3, None, nrm)      # either output may be NULL
    NOISE(1, 0, 2, 3, words, None)


def test_restated_H_is_the_oracles_on_c1():
    g = util.c1_arrays()
    for kind in ("constant", "analytic"):
        with lm_rules._Jacobians(kind):
            H, _b, _err, _idx = oracle.linearize(util.to_oracle(g))
        S = posterior.System(g, jacobian=kind)
        assert S.H.shape == H.shape
        assert np.abs(S.H - H).max() <= 1e-9 * np.abs(H).max(), kind


@functools.lru_cache(maxsize=None)
def c1_statistics():
    """The restatement's own samples on c1 at its start (analytic Jacobians), the seed and K of the GPU statistics test."""
    g = util.c1_arrays()
    S = posterior.System(g, jacobian="analytic")
    d, _b = S.samples(posterior.SEED_STAT, posterior.K_STAT)
    return S, d


def test_statistical_bounds_hold_for_the_restatement():
    S, d = c1_statistics()
    K = posterior.K_STAT
    var = (d * d).mean(axis=0)
    ref = S.inverse_diagonal()
    mask = np.arange(3)[None, :] < S.dims[:, None]
    ratio = var[mask] / ref[mask]
    assert np.abs(ratio - 1).max() <= posterior.BOUND * np.sqrt(2.0 / K), (ratio.min(), ratio.max())
    x = S.packed(d)
    q = np.einsum("kn,nm,km->k", x, S.H, x).mean()
    n = S.H.shape[0]
    assert abs(q - n) <= posterior.BOUND * np.sqrt(2.0 * n / K), (q, n)


def test_five_class_graph_has_the_cases_and_a_regular_H():
    g, edges = posterior.five_class_graph()
    assert sorted(set(g.e_type.tolist())) == [0, 1, 2, 3, 4]
    assert (g.e_inf[edges[0]] == 0).all() and len(g.fixed) == 3 and g.fixed[0] == g.fixed[1]
    assert g.v_type[np.flatnonzero(g.v_id == g.fixed[2])[0]] == 1
    assert len(posterior.single_observation_landmarks(g)) > 0
    for kind in ("constant", "analytic"):
        S = posterior.System(g, posterior.ROBUST, kind)
        assert np.linalg.cond(S.H) < 1e12
        assert sorted(set(S.gauge[S.gauge > 0].tolist())) == [1e6, 2e6]
        # sample k does not depend on K, and another seed gives other samples
        d5, _ = S.samples(posterior.SEED, 5)
        d3, _ = S.samples(posterior.SEED, 3)
        assert np.array_equal(d5[:3], d3)
        assert (S.samples(posterior.SEED + 1, 3)[0] != d3)[:, np.arange(3)[None, :] < S.dims[:, None]].all()
