"""The Metropolis-Hastings plumbing of the host test ABI without a GPU: host_mh_run_analytic runs the sampler's scalar path
over a correlated Gaussian's log-density through the settings builder and the output record every MH entry point of
host_capi.cpp uses, so that the chain, sample and coordinate strides of their outputs are checked on any machine."""
import numpy as np
import pytest

MEAN = np.array([0.5, -1.0])
PRECISION = np.array([[2.0, 0.6], [0.6, 1.0]])
STARTS = np.array([[0.0, 0.0], [1.5, -2.0], [-1.0, 0.5]])
# 7 samples (t = 0, 4, .., 24): chain, sample and coordinate strides all differ and 7 divides neither 25 nor 24
RUN = dict(seed=11, iterations=25, burn_in=5, adaptation_period=10, thinning=4)
ARRAYS = ("accepted", "best_value", "best", "final_scale", "accept_trace", "samples", "sample_values", "final_cov")


def _density(x):
    d = np.asarray(x) - MEAN
    return -0.5 * np.einsum("...i,ij,...j->...", d, PRECISION, d)


@pytest.fixture(scope="module")
def three(mm):
    return mm.hostabi.mh_analytic(MEAN, PRECISION, STARTS, **RUN)


def test_shapes_and_layout(three):
    assert set(three) == set(ARRAYS)
    assert three["samples"].shape == (3, 7, 2)
    assert np.array_equal(three["samples"][:, 0], STARTS)
    # a dozen flops: rounding moves the value by ~1e-16, a wrong stride by order one
    np.testing.assert_allclose(three["sample_values"], _density(three["samples"]), rtol=1e-12, atol=0.0)
    assert three["accept_trace"].shape == (3, 24) and three["accept_trace"].dtype == np.uint8
    assert np.array_equal(three["accepted"], three["accept_trace"].sum(axis=1))
    np.testing.assert_allclose(three["best_value"], _density(three["best"]), rtol=1e-12, atol=0.0)
    assert np.all(three["best_value"] >= three["sample_values"].max(axis=1))
    assert three["final_cov"].shape == (3, 2, 2)
    assert np.array_equal(three["final_cov"], three["final_cov"].transpose(0, 2, 1))
    assert np.all(three["final_scale"] > 0.0)


def test_chain_c_is_the_single_chain_run_with_seed_plus_c(mm, three):
    for c in range(3):
        one = mm.hostabi.mh_analytic(MEAN, PRECISION, STARTS[c], **dict(RUN, seed=RUN["seed"] + c))
        for k in ARRAYS:
            assert one[k].shape == three[k][c:c + 1].shape, k
            assert np.array_equal(one[k][0], three[k][c]), (k, c)


def test_without_the_trace_the_rest_is_unchanged(mm, three):
    bare = mm.hostabi.mh_analytic(MEAN, PRECISION, STARTS, want_trace=False, **RUN)
    assert bare["accept_trace"] is None
    for k in ARRAYS:
        if k != "accept_trace":
            assert np.array_equal(bare[k], three[k]), k
