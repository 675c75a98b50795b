"""tests/march_ref.py before the kernels are held to it (tests/test_gpu_march_kernels.py): the float64 reference
against torch float64 autograd of the same loop written with torch ops, and the input generators' conditions (no
near-ties, the clamp and the clipped / border lookups covered), checked on the float64 reference alone."""
import numpy as np
import pytest
import torch

import march_ref as mr

F64 = torch.float64

# every generator call the GPU tests make: (generator, arguments)
FORWARD_CASES = [(H, W, sb, n, steps) for (H, W) in ((5, 7), (8, 8))
                 for (sb, n) in ((1, 1), (1, 15), (1, 17), (3, 65), (2, 300)) for steps in (1, 10)]
FORWARD_CASES += [(5, 7, 1, 16, 2), (8, 8, 2, 63, 2)]
SYNTHETIC_CASES = [(5, 7, 1, 1, 1), (5, 7, 1, 15, 2), (8, 8, 1, 16, 10), (5, 7, 1, 17, 1), (5, 7, 2, 63, 2),
                   (8, 8, 3, 65, 10), (5, 7, 2, 300, 10)]
SATURATION_RAYS = (1024, 1025)


# ------------------------------------------------------------------------------ the reference against autograd
def _torch_lookup(view, x):
    """The lookup with torch ops (differentiable in x through the weights; torch.clamp passes no gradient where it
    clips, floor none at all: grid_sample's border / align_corners=True backward)."""
    t64 = lambda a: torch.tensor(np.asarray(a, np.float32).astype(np.float64))  # noqa: E731
    P, f, c = t64(view["poses"]), t64(view["focal"]), t64(view["c"])
    scale = t64(view["latent_scaling"]) / t64(view["image_shape"])
    H, W = view["H"], view["W"]
    xc = x @ P[:, :3].t() + P[:, 3]
    u = -xc[:, 0] / xc[:, 2] * f[0] + c[0]
    v = -xc[:, 1] / xc[:, 2] * f[1] + c[1]
    ix = (u * scale[0] * 0.5 * (W - 1)).clamp(0, W - 1)
    iy = (v * scale[1] * 0.5 * (H - 1)).clamp(0, H - 1)
    X0, Y0 = ix.detach().floor().long(), iy.detach().floor().long()
    X1, Y1 = (X0 + 1).clamp(max=W - 1), (Y0 + 1).clamp(max=H - 1)
    wx1, wy1 = ix - X0, iy - Y0
    wx0, wy0 = 1 - wx1, 1 - wy1
    return (Y0 * W + X0, Y0 * W + X1, Y1 * W + X0, Y1 * W + X1), (wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1)


def _torch_march(case, pos_grad):
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    leaves = {k: t64(getattr(case, k)).requires_grad_(True) for k in ("tables", "w_hh", "b_ih", "b_hh", "w_out",
                                                                       "b_out")}
    ro, rd, d0 = t64(case.ro), t64(case.rd), t64(case.d0)
    n, nps = case.n, case.n_per_scene
    x = ro + rd * d0[:, None]
    h, c = torch.zeros(n, 16, dtype=F64), torch.zeros(n, 16, dtype=F64)
    states = []
    for _ in range(case.steps):
        rows = []
        for sc, view in enumerate(case.views):
            xs = x[sc * nps:(sc + 1) * nps]
            tex, w = _torch_lookup(view, xs if pos_grad else xs.detach())
            rows.append(sum(leaves["tables"][sc][tex[q]] * w[q][:, None] for q in range(4)))
        g = torch.cat(rows) + leaves["b_ih"] + leaves["b_hh"] + h @ leaves["w_hh"].t()
        i, f, gg, o = g[:, :16].sigmoid(), g[:, 16:32].sigmoid(), g[:, 32:48].tanh(), g[:, 48:].sigmoid()
        c = f * c + i * gg
        h = o * c.tanh()
        h.register_hook(lambda gr: gr.clamp(-10, 10))
        states.append(torch.cat([h, c, i, f, gg, o], 1).detach())
        x = x + rd * (h @ leaves["w_out"] + leaves["b_out"])[:, None]
    return x, torch.stack(states), leaves


@pytest.mark.parametrize("pos_grad", [1, 0])
def test_reference_matches_torch_autograd(pos_grad):
    case = mr.forward_case(5, 7, 2, 33, 3)
    world, trace, state = mr.forward(case)
    tw, tstate, leaves = _torch_march(case, pos_grad)
    np.testing.assert_allclose(world, tw.detach().numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(state, tstate.numpy(), rtol=0, atol=1e-12)
    (tw * torch.tensor(case.gw.astype(np.float64))).sum().backward()
    ref = mr.backward(case, trace, state, case.gw, pos_grad)
    clamped = np.abs(ref.dh_pre) > mr.CLAMP
    assert 0.05 <= clamped.mean() <= 0.95, clamped.mean()
    got = {"d_tables": leaves["tables"].grad.numpy(), "dW_hh": leaves["w_hh"].grad.numpy().ravel(),
           "db": leaves["b_ih"].grad.numpy(), "dw_out": leaves["w_out"].grad.numpy(),
           "db_out": leaves["b_out"].grad.numpy()}
    np.testing.assert_array_equal(leaves["b_ih"].grad.numpy(), leaves["b_hh"].grad.numpy())
    assert mr.rel_S(got["d_tables"], ref.d_tables, ref.S_tables) <= 1e-10
    untouched = ref.S_tables == 0
    assert untouched.any() and not got["d_tables"][untouched].any() and not ref.d_tables[untouched].any()
    for name, sl in mr.BLOCKS.items():
        assert (ref.S_grads[sl] > 0).all(), name
        assert mr.rel_S(got[name], ref.d_grads[sl], ref.S_grads[sl]) <= 1e-10, name
    # the position gradient matters at these inputs (so the pos_grad = 1 agreement above tests it)
    if pos_grad:
        off = mr.backward(case, trace, state, case.gw, 0)
        assert mr.rel_S(off.d_tables, ref.d_tables, ref.S_tables) > 1e-3


def test_float32_reference_is_a_float32_run():
    """The yardstick runs in float32 end to end (no silent promotion) and lands near the float64 run."""
    case = mr.forward_case(5, 7, 2, 33, 3)
    w32, t32, s32 = mr.forward(case, np.float32)
    assert w32.dtype == t32.dtype == s32.dtype == np.float32
    b32 = mr.backward(case, t32, s32, case.gw, 1, np.float32)
    assert b32.d_tables.dtype == b32.d_grads.dtype == b32.S_tables.dtype == np.float32
    L = mr.lookup(case.views[0], t32[0][:33])
    assert L.w.dtype == L.dix.dtype == L.ixr.dtype == np.float32
    _, _, s64 = mr.forward(case)
    err = float(np.abs(s32 - s64).max())
    assert 0 < err < 1e-4, err


# ------------------------------------------------------------------------------------------ input conditions
def _check_coords(case, trace, coverage=True):
    ixr, iyr = mr.case_lookups(case, trace)
    assert mr.coords_ok(ixr, iyr, case.H, case.W).all()   # zero exclusions
    clip_x = (ixr <= 0) | (ixr >= case.W - 1)
    clip_y = (iyr <= 0) | (iyr >= case.H - 1)
    last = (ixr >= case.W - 1) | (iyr >= case.H - 1)
    if coverage:
        assert clip_x.mean() >= 0.10 and clip_y.mean() >= 0.10 and last.mean() >= 0.10, \
            (clip_x.mean(), clip_y.mean(), last.mean())
    return clip_x.mean(), clip_y.mean(), last.mean()


def _check_clamp(case, trace, state):
    for pos_grad in (1, 0):
        dh = mr.backward(case, trace, state, case.gw, pos_grad, scatter=False).dh_pre
        assert mr.dh_ok(dh).all()   # zero exclusions
        clamped = (np.abs(dh) > mr.CLAMP).mean()
        assert 0.05 <= clamped <= 0.95, (pos_grad, clamped)


def _pooled(cases, make):
    """The coverage shares of a generator's small cases (one ray has no 10 % of anything) are taken over the
    generator's cases of one latent size together; the near-tie conditions hold for every case by itself."""
    by_latent = {}
    for args in cases:
        case, trace = make(args)
        ixr, iyr = mr.case_lookups(case, trace)
        by_latent.setdefault(args[:2], []).append((ixr.ravel(), iyr.ravel()))
    for (H, W), parts in by_latent.items():
        ixr, iyr = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        assert ((ixr <= 0) | (ixr >= W - 1)).mean() >= 0.10
        assert ((iyr <= 0) | (iyr >= H - 1)).mean() >= 0.10
        assert ((ixr >= W - 1) | (iyr >= H - 1)).mean() >= 0.10


@pytest.mark.parametrize("args", FORWARD_CASES, ids=lambda a: "x".join(map(str, a)))
def test_forward_case_conditions(args):
    case = mr.forward_case(*args)
    _, trace, state = mr.forward(case)
    big = case.n * case.steps >= 100
    _check_coords(case, trace, coverage=big)
    if big:
        _check_clamp(case, trace, state)
    else:
        for pos_grad in (1, 0):
            assert mr.dh_ok(mr.backward(case, trace, state, case.gw, pos_grad, scatter=False).dh_pre).all()


@pytest.mark.parametrize("args", SYNTHETIC_CASES, ids=lambda a: "x".join(map(str, a)))
def test_synthetic_case_conditions(args):
    case = mr.synthetic_case(*args)
    big = case.n * case.steps >= 100
    _check_coords(case, case.trace, coverage=big)
    if big:
        _check_clamp(case, case.trace, case.state)
    else:
        for pos_grad in (1, 0):
            assert mr.dh_ok(mr.backward(case, case.trace, case.state, case.gw, pos_grad,
                                        scatter=False).dh_pre).all()


def test_small_cases_cover_together():
    _pooled([a for a in FORWARD_CASES if a[2] * a[3] * a[4] < 100], lambda a: (mr.forward_case(*a),
                                                                                 mr.forward(mr.forward_case(*a))[1]))
    _pooled([a for a in SYNTHETIC_CASES if a[2] * a[3] * a[4] < 100], lambda a: (mr.synthetic_case(*a),
                                                                                   mr.synthetic_case(*a).trace))


def test_two_group_case_conditions():
    case = mr.two_group_case()
    _check_coords(case, case.trace)
    ref = mr.backward(case, case.trace, case.state, case.gw, 1)
    assert np.abs(ref.dh_pre).max() < mr.CLAMP * (1 - mr.TIE)          # the clamp is off: dg linear in grad_world
    assert mr.max_dg_exponent_ok(ref.max_dg)
    # the groups' texels are disjoint (columns 0 .. 3 / 4 .. 6), and B lies 2^-30 below A
    col = np.arange(case.H * case.W) % case.W
    A = mr.backward(case, case.trace, case.state, np.where(np.arange(case.n)[:, None] < mr.GROUP, case.gw, 0), 1)
    B = mr.backward(case, case.trace, case.state, np.where(np.arange(case.n)[:, None] >= mr.GROUP, case.gw, 0), 1)
    assert not A.S_tables[0][col >= 4].any() and not B.S_tables[0][col < 4].any()
    assert B.S_tables[0][col >= 4].any(1).sum() >= 10 and A.S_tables[0][col < 4].any(1).sum() >= 10
    assert 2.0 ** -33 < B.max_dg / A.max_dg < 2.0 ** -27
    # the fixed-point grid leaves every group-B entry a relative accuracy the GPU test can decide against 2^-10:
    # n_i 2^(cbits + e - 63) is below 2^-12 of S_i
    on = (col >= 4)[:, None] & (ref.S_tables[0] > 0)
    grid = ref.count[0][:, None] * 2.0 ** (mr.cbits_of(1, case.n) + int(np.frexp(ref.max_dg)[1]) - 63)
    assert (np.broadcast_to(grid, on.shape)[on] / ref.S_tables[0][on]).max() < 2.0 ** -12
    # dropping any one group-A ray (the non-finite gradient test does) leaves the exponent unambiguous
    for r in range(mr.GROUP):
        gw = case.gw.copy()
        gw[r] = 0
        assert mr.max_dg_exponent_ok(mr.backward(case, case.trace, case.state, gw, 1, scatter=False).max_dg)


@pytest.mark.parametrize("n", SATURATION_RAYS)
def test_saturation_case_conditions(n):
    case = mr.saturation_case(n)
    _check_coords(case, case.trace)
    L = mr.lookup(case.views[0], case.trace[0].astype(np.float64))
    assert (L.w == np.array([1.0, 0.0, 0.0, 0.0])).all() and (L.tex == case.H * case.W - 1).all()
    assert (mr.lookup(case.views[0], case.trace[0]).w == np.array([1, 0, 0, 0], np.float32)).all()
    ref = mr.backward(case, case.trace, case.state, case.gw, 1)
    assert np.abs(ref.dh_pre).max() < mr.CLAMP * (1 - mr.TIE) and mr.max_dg_exponent_ok(ref.max_dg)
    assert mr.cbits_of(1, n) == (12 if n == 1024 else 13)
    assert (ref.count[0, -1] == n) and ref.count.sum() == n
    # same-sign contributions: the texel's entries are n * dg
    one = mr.backward(mr.saturation_case(1), case.trace[:, :1], case.state[:, :1], case.gw[:1], 1)
    np.testing.assert_allclose(ref.d_tables[0, -1], n * one.d_tables[0, -1], rtol=1e-12)
    assert (ref.S_tables[0, -1] == np.abs(ref.d_tables[0, -1])).all()
    rows = np.arange(mr.GATES) // mr.HID != 1   # the forget gate's gradient is 0 at step 0 (c_prev = 0)
    assert ref.d_tables[0, -1][rows].all() and not ref.d_tables[0, -1][~rows].any()
