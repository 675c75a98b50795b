"""tests/bn_ref.py (the float64 reference the BatchNorm training kernels are held to) against torch float64: the
reference's pieces composed into one relu(bn(x)) -> linear forward and its backward over rows split into 64-row
workgroups, against torch.nn.functional.batch_norm(training=True) + autograd. Output, running statistics, dgamma,
dbeta within 1e-12 of each tensor's largest value, dx within 1e-12 of its column's terms. Column 0 has mean / std =
4096, column 1 is constant."""
import numpy as np
import pytest
import torch

import bn_ref

EPS, MOMENTUM = 1e-5, 0.1
C, H = 6, 5


def _inputs(M, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, C)) * np.array([0.37, 1.0, 1.0, 5.0, 0.01, 2.0]) + np.array([0, 0, 0.5, -3, 8, 0])
    x[:, 0] += 0.37 * 4096                      # mean / std = 4096
    x[:, 1] = 3.0                               # a constant column (its sums are exact)
    return dict(x=x, W=rng.standard_normal((H, C)), b=rng.standard_normal(H), w=rng.standard_normal((M, H)),
                gamma=rng.uniform(0.5, 1.5, C), beta=rng.uniform(0.1, 0.3, C) * rng.choice([-1.0, 1.0], C),
                rm=rng.standard_normal(C), rv=rng.uniform(0.5, 2.0, C))


def _ref(d, M):
    """Forward and backward from bn_ref's functions alone, the statistics through the per-workgroup partials."""
    p0, p1 = bn_ref.group_stats(d["x"])
    mu, invstd, scale, rm, rv = bn_ref.stats_from_partials(p0, p1, M, d["gamma"], EPS, MOMENTUM, d["rm"], d["rv"])
    _, out, _ = bn_ref.layer_fwd(d["x"], d["W"], d["b"], (mu, scale, d["beta"]))
    # d loss / d out = w (loss = sum out * w); fc^T with the relu mask, then the BatchNorm backward
    _, gp, _, (s1, s2) = bn_ref.layer_bwd(d["w"], d["W"], d["x"], (mu, invstd, scale, d["beta"]))
    zeros = np.zeros(C)
    coef, m1, m2, dgamma, dbeta = bn_ref.grad_stats_from_partials(s1, s2, M, d["gamma"], invstd, zeros, zeros)
    dx = bn_ref.grad_rows(gp, d["x"], None, coef, m1, m2, mu, invstd)
    # dx = coef * (gp - m1 - xhat * m2) cancels (to ~0 at M = 2): its error is measured against its terms' size
    return dict(out=out, rm=rm, rv=rv, dx=dx, dgamma=dgamma, dbeta=dbeta), np.abs(coef) * np.abs(gp).max(0)


def _torch(d):
    T = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))  # noqa: E731
    x, gamma, beta = (T(d[k]).requires_grad_(True) for k in ("x", "gamma", "beta"))
    rm, rv = T(d["rm"]), T(d["rv"])
    y = torch.nn.functional.batch_norm(x, rm, rv, gamma, beta, True, MOMENTUM, EPS)
    out = torch.nn.functional.linear(torch.relu(y), T(d["W"]), T(d["b"]))
    (out * T(d["w"])).sum().backward()
    return {k: v.detach().numpy() for k, v in dict(out=out, rm=rm, rv=rv, dx=x.grad, dgamma=gamma.grad,
                                                   dbeta=beta.grad).items()}


@pytest.mark.parametrize("M", [2, 65, 1025])
def test_bn_ref_matches_torch_float64(M):
    d = _inputs(M, seed=M)
    (got, dx_scale), want = _ref(d, M), _torch(d)
    for k in want:
        # dx column by column (the constant column's invstd = 1 / sqrt(eps) would hide the others)
        s = dx_scale if k == "dx" else np.abs(want[k]).max()
        s = np.where(s > 0, s, 1.0)
        err = float((np.abs(got[k] - want[k]) / s).max())
        print(f"bn_ref vs torch float64, M={M}, {k}: {err:.2e} (bar 1e-12) of {float(np.min(s)):.2e}")
        assert err <= 1e-12, (k, err)


def test_bn_ref_partials_do_not_change_the_statistics():
    """The statistics combined from 64-row partials are the statistics of the rows themselves, the last workgroup
    of 1 row included, and the combine is indifferent to the pivot at mean / std = 4096."""
    d = _inputs(129, seed=7)
    p0, p1 = bn_ref.group_stats(d["x"])
    assert p0.shape == (3, C) and np.array_equal(bn_ref.group_sizes(129), [64, 64, 1])
    assert np.array_equal(p0[2], d["x"][128]) and not p1[2].any()
    mu, invstd, _, _, _ = bn_ref.stats_from_partials(p0, p1, 129, d["gamma"], EPS, MOMENTUM)
    x = d["x"].astype(np.longdouble)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    assert np.abs(mu - mean).max() <= 1e-15 * np.abs(mean).max()
    assert (np.abs(invstd - 1 / np.sqrt(var + EPS)) * np.sqrt(var + EPS)).max() <= 1e-14
    assert abs(invstd[1] * np.sqrt(EPS) - 1) <= 1e-15     # the constant column: M2 = 0 exactly
