"""The numpy reference of weighted CP (tests/wls_ref.py) checked against the mathematics it restates: Kiers'
majorization inequality with equality at the supporting point, the EM imputation as its 0/1 case, and a loss
that never rises along the MM-ALS loop."""
import numpy as np

import wls_ref as R


def rand_factors(shape, r, seed, lo=0.0):
    g = np.random.default_rng(seed)
    return [g.uniform(lo, 1.0, (n, r)) for n in shape]


def test_majorization_inequality_with_equality_at_the_supporting_point():
    g = np.random.default_rng(0)
    shape = (7, 6, 5)
    for trial in range(20):
        x = g.normal(size=shape)
        h = g.uniform(size=shape)
        h[g.uniform(size=shape) < 0.1] = 0.0
        h[g.uniform(size=shape) < 0.1] = 1.0
        m0 = R.cp_model(rand_factors(shape, 3, 10 + trial, -1.0))
        l0 = R.loss(x, h, m0)
        assert abs(R.majorizer(x, h, m0, m0) - l0) <= 1e-13 * l0
        for k in range(5):
            m = m0 + g.normal(size=shape) * 10.0 ** (-k)
            assert R.loss(x, h, m) <= R.majorizer(x, h, m0, m) * (1 + 1e-14)


def test_special_weights_follow_the_rule():
    m = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    x = np.array([2.0, np.nan, np.inf, 1.0, 7.0, 0.0])
    h = np.array([2.0, -1.0, np.nan, 0.25, 1.0, 0.0])
    z, l = R.step(x, h, m)
    assert np.array_equal(z, [2.0, 2.0, 3.0, 4.0 + 0.25 * (1.0 - 4.0), 7.0, 6.0])
    assert l == 1.0 + 0.25 * 9.0 + 4.0


def test_zero_one_weights_are_the_em_imputation():
    g = np.random.default_rng(1)
    shape = (6, 5, 4, 3)
    x = g.normal(size=shape)
    mask = g.uniform(size=shape) >= 0.3
    m = R.cp_model(rand_factors(shape, 2, 3, -1.0))
    z, l = R.step(np.where(mask, x, np.nan), mask.astype(np.float64), m)
    assert np.array_equal(z, np.where(mask, x, m))
    assert l == float(np.sum(((x - m) ** 2)[mask]))


def test_loss_never_rises_over_200_iterations():
    g = np.random.default_rng(2)
    shape, r = (8, 7, 6), 3
    x = R.cp_model(rand_factors(shape, r, 4))
    sigma = np.where(g.uniform(size=shape) < 0.3, 1.0, 0.01)
    x = x + sigma * g.normal(size=shape)
    h = (sigma.min() / sigma) ** 2
    looks = []
    R.mm_als(x, h, rand_factors(shape, r, 5), 200, look=lambda k, l: looks.append(l))
    assert len(looks) == 200
    rise = max((b - a) / a for a, b in zip(looks, looks[1:]))
    assert rise <= 1e-12, rise
    assert looks[-1] < 0.5 * looks[0]
