"""The numpy reference of robust CP (tests/huber_ref.py) checked against what it claims: with c = inf the step
is the weighted step's, the majorizer lies above Huber's loss and touches it at the current model, the MM-ALS
loop never raises the loss (also with the working tensor rounded to fp32), and the quantile follows its
definition on hand-made arrays."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import huber_ref  # noqa: E402
import wls_ref  # noqa: E402


def _problem(seed, shape=(7, 6, 5), R=2):
    g = np.random.default_rng(seed)
    W = [g.uniform(0.0, 1.0, (n, R)) for n in shape]
    x = wls_ref.cp_model(W) + 0.05 * g.normal(size=shape)
    bad = g.uniform(size=shape) < 0.1
    x = x + bad * g.choice([-1.0, 1.0], size=shape) * g.uniform(0.5, 2.0, size=shape)
    h = g.uniform(0.01, 0.99, size=shape)
    u = g.uniform(size=shape)
    h[u < 0.1] = 0.0
    h[u > 0.8] = 1.0
    h[(u > 0.1) & (u < 0.15)] = 2.0
    return g, W, x, h


def test_rho():
    assert np.array_equal(huber_ref.rho([0.0, 0.5, -1.0, 3.0, -3.0], 1.0), [0.0, 0.25, 1.0, 5.0, 5.0])
    assert np.array_equal(huber_ref.rho([2.0, -3.0], np.inf), [4.0, 9.0])


def test_step_without_clipping_is_the_weighted_step_exactly():
    g, W, x, h = _problem(0)
    m = wls_ref.cp_model([w + 0.1 * g.normal(size=w.shape) for w in W])
    h[0, 0, 0] = np.nan
    h[0, 0, 1] = -1.0
    x[0, 0, 0] = np.inf
    x[0, 0, 1] = np.nan
    z, l, n = huber_ref.step(x, h, m, np.inf)
    zw, lw = wls_ref.step(x, h, m)
    assert z.tobytes() == zw.tobytes() and l == lw and n == 0
    xx = np.where(np.isfinite(x), x, 0.0)
    z1, l1, n1 = huber_ref.step(xx, None, m, np.inf)
    assert np.array_equal(z1, xx) and l1 == float(np.sum((xx - m) * (xx - m))) and n1 == 0


def test_step_rule_by_rule():
    m = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    x = np.array([1.25, 3.0, -2.0, 3.0, np.inf, np.nan])
    h = np.array([1.0, 1.0, 0.5, 0.0, 2.0, -1.0])
    z, l, n = huber_ref.step(x, h, m, 0.5)
    assert np.array_equal(z, [1.25, 1.5, 0.75, 1.0, 1.5, 1.0])
    assert n == 3 and l == np.inf
    z, l, n = huber_ref.step(x[:4], h[:4], m[:4], 0.5)
    assert l == 0.0625 + 0.5 * (4.0 - 0.5) + 0.5 * 0.5 * (6.0 - 0.5) and n == 2


def test_majorizer_lies_above_the_loss_and_touches_it():
    g, W, x, h = _problem(1)
    m0 = wls_ref.cp_model(W)
    c = float(np.median(np.abs(x - m0)))
    for hh in (h, None):
        l0 = huber_ref.loss(x, hh, m0, c)
        assert abs(huber_ref.majorizer(x, hh, m0, m0, c) - l0) <= 1e-12 * l0
        for _ in range(100):
            m = m0 + g.normal(size=m0.shape) * g.choice([1e-3, 0.1, 1.0, 10.0])
            assert huber_ref.majorizer(x, hh, m0, m, c) >= huber_ref.loss(x, hh, m, c) * (1 - 1e-12)


def test_mm_als_never_raises_the_loss():
    for seed, store in ((2, None), (3, lambda z: z.astype(np.float32).astype(np.float64))):
        g, W, x, h = _problem(seed)
        W0 = [g.uniform(0.0, 1.0, w.shape) for w in W]
        for hh in (h, None):
            c = 1.345 * 1.4826 * float(np.median(np.abs(x - wls_ref.cp_model(W0))))
            looks = []
            huber_ref.mm_als(x, hh, W0, 40, c, store=store, look=lambda k, l, n: looks.append(l))
            rise = max((b - a) / a for a, b in zip(looks, looks[1:]))
            assert rise <= 1e-9 and looks[-1] < 0.9 * looks[0], (seed, rise, looks[0], looks[-1])


def test_quantile_of_hand_made_arrays():
    m = np.zeros(8)
    x = np.array([3.0, -1.0, 0.0, 1.0, -0.0, 2.0, 1.0, -3.0])     # |.| sorted: 0 0 1 1 1 2 3 3
    want = {0.0: 0.0, 0.25: 0.0, 0.26: 1.0, 0.5: 1.0, 0.625: 1.0, 0.63: 2.0, 0.9: 3.0, 1.0: 3.0}
    for p, v in want.items():
        assert huber_ref.quantile(x, None, m, p) == (v, 8), p
    h = np.array([1.0, 0.0, 0.5, -1.0, np.nan, 2.0, 1e-30, 1.0])  # keeps 3 0 2 1 3 -> 0 1 2 3 3
    assert huber_ref.quantile(x, h, m, 0.5) == (2.0, 5)
    assert huber_ref.quantile(x, h, m, 0.2) == (0.0, 5) and huber_ref.quantile(x, h, m, 0.21) == (1.0, 5)
    v, n = huber_ref.quantile(x, np.zeros(8), m, 0.5)
    assert math.isnan(v) and n == 0
    y = np.array([1.0, np.inf, np.nan, 2.0])                      # sorted: 1 2 inf nan
    assert huber_ref.quantile(y, None, 0.0, 0.75) == (np.inf, 4)
    v, n = huber_ref.quantile(y, None, 0.0, 1.0)
    assert math.isnan(v) and n == 4
    assert huber_ref.quantile(y, None, 0.0, 0.5) == (2.0, 4)
    # rounded to fp32 before it is ranked: 1 + 2^-30 and 1 are one key
    assert huber_ref.quantile(np.array([1.0 + 2.0 ** -30, 1.0]), None, 0.0, 1.0) == (1.0, 2)
    assert huber_ref.quantile(np.array([5.0]), None, 1.0, 0.3) == (4.0, 1)
