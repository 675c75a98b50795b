"""Reference of the LSTM march's training kernels (csrc/raymarch.hip: avr_raymarch_train / avr_raymarch_bwd) in
numpy, in a dtype the caller passes: np.float64 is the reference the kernels are held to, np.float32 the yardstick
(the same recursion in the kernels' own number format). Nothing here imports avr: the operation is restated.

A view is a dict of the fp32 fields of avr_view_desc: poses (3, 4), focal (2), c (2), image_shape (2),
latent_scaling (2), H, W. Tables are (n_scenes, H*W, 64) gate projections; the state of a ray and step is
h, c, i, f, g, o, 16 values each.

The second half holds the seeded input generators that tests/test_march_ref_cpu.py (their conditions) and
tests/test_gpu_march_kernels.py (the kernels) share. A generator draws more rays than it needs and keeps the first
ones whose float64 run has no near-tie (a lookup coordinate within TIE of an integer or a clip edge, a pre-clamp
|dh| within TIE relative of 10): every ray is independent of the others, so the kept rays are a valid input of their
own, and no element of any output is left out of a comparison."""
import functools
from types import SimpleNamespace

import numpy as np

HID = 16
GATES = 4 * HID
STATE = 6 * HID
N_GRADS = GATES * HID + GATES + HID + 1
BLOCKS = {"dW_hh": slice(0, 1024), "db": slice(1024, 1088), "dw_out": slice(1088, 1104), "db_out": slice(1104, 1105)}
TIE = 1e-3
CLAMP = 10.0


def _sigmoid(x):
    return 1 / (1 + np.exp(-x))


def _view_terms(view, T):
    P = np.asarray(view["poses"], np.float32).reshape(3, 4).astype(T)
    f, c = np.asarray(view["focal"], np.float32).astype(T), np.asarray(view["c"], np.float32).astype(T)
    scale = np.asarray(view["latent_scaling"], np.float32).astype(T) / np.asarray(view["image_shape"],
                                                                                 np.float32).astype(T)
    return P[:, :3], P[:, 3], f, c, scale


def lookup(view, pts):
    """lookup_grad of raymarch.hip at pts (n, 3), in pts' dtype: xc = R x + t, pinhole uv, uv * scale - 1,
    grid_sample bilinear / border / align_corners=True. Returns tex (n, 4) and w (n, 4) in the order
    (Y0, X0), (Y0, X1), (Y1, X0), (Y1, X1), the 1-D weights wx0, wx1, wy0, wy1, dix and diy (n, 3) = d ix / d xc and
    d iy / d xc (zero where the coordinate was clipped) and the unclipped ixr, iyr."""
    T = pts.dtype.type
    R, t, f, c, scale = _view_terms(view, T)
    H, W = int(view["H"]), int(view["W"])
    x0, x1, x2 = pts[:, 0], pts[:, 1], pts[:, 2]
    xc = [((R[i, 0] * x0 + R[i, 1] * x1) + R[i, 2] * x2) + t[i] for i in range(3)]
    u = (-xc[0] / xc[2]) * f[0] + c[0]
    v = (-xc[1] / xc[2]) * f[1] + c[1]
    gx, gy = u * scale[0] - T(1), v * scale[1] - T(1)
    ixr = ((gx + T(1)) / T(2)) * T(W - 1)
    iyr = ((gy + T(1)) / T(2)) * T(H - 1)
    ix, iy = np.clip(ixr, T(0), T(W - 1)), np.clip(iyr, T(0), T(H - 1))
    fx0, fy0 = np.floor(ix), np.floor(iy)
    wx1, wy1 = ix - fx0, iy - fy0
    wx0, wy0 = (fx0 + T(1)) - ix, (fy0 + T(1)) - iy
    X0, Y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    X1, Y1 = np.minimum(X0 + 1, W - 1), np.minimum(Y0 + 1, H - 1)
    tex = np.stack([Y0 * W + X0, Y0 * W + X1, Y1 * W + X0, Y1 * W + X1], 1)
    w = np.stack([wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1], 1)
    cx = (ixr > 0) & (ixr < W - 1)
    cy = (iyr > 0) & (iyr < H - 1)
    ax = T(0.5) * T(W - 1) * scale[0] * f[0]
    ay = T(0.5) * T(H - 1) * scale[1] * f[1]
    iz = T(1) / xc[2]
    zero = np.zeros_like(iz)
    dix = np.stack([np.where(cx, -ax * iz, zero), zero, np.where(cx, ax * xc[0] * iz * iz, zero)], 1)
    diy = np.stack([zero, np.where(cy, -ay * iz, zero), np.where(cy, ay * xc[1] * iz * iz, zero)], 1)
    return SimpleNamespace(tex=tex, w=w, wx0=wx0, wx1=wx1, wy0=wy0, wy1=wy1, dix=dix, diy=diy, ixr=ixr, iyr=iyr)


def _blend(tb, L):
    return ((tb[L.tex[:, 0]] * L.w[:, 0:1] + tb[L.tex[:, 1]] * L.w[:, 1:2]) + tb[L.tex[:, 2]] * L.w[:, 2:3]) \
        + tb[L.tex[:, 3]] * L.w[:, 3:4]


def march_forward(views, tables, w_hh, b_ih, b_hh, w_out, b_out, ro, rd, d0, n_per_scene, steps, dtype=np.float64):
    """avr_raymarch_train: world (n, 3), trace (steps + 1, n, 3), state (steps, n, 96), computed in dtype."""
    T = np.dtype(dtype).type
    tables, w_hh, b_ih, b_hh, w_out, b_out, ro, rd, d0 = (np.asarray(a).astype(T) for a in
                                                          (tables, w_hh, b_ih, b_hh, w_out, b_out, ro, rd, d0))
    n = ro.shape[0]
    w_out, b_out = w_out.reshape(HID), b_out.reshape(())
    bias = b_ih + b_hh
    x = ro + rd * d0.reshape(n, 1)
    trace = np.empty((steps + 1, n, 3), T)
    state = np.empty((steps, n, STATE), T)
    trace[0] = x
    h, c = np.zeros((n, HID), T), np.zeros((n, HID), T)
    with np.errstate(all="ignore"):
        for s in range(steps):
            g = np.empty((n, GATES), T)
            for sc, view in enumerate(views):
                sl = slice(sc * n_per_scene, (sc + 1) * n_per_scene)
                g[sl] = _blend(tables[sc], lookup(view, x[sl])) + bias
            g = g + h @ w_hh.T
            ig, fg = _sigmoid(g[:, :HID]), _sigmoid(g[:, HID:2 * HID])
            gg, og = np.tanh(g[:, 2 * HID:3 * HID]), _sigmoid(g[:, 3 * HID:])
            c = fg * c + ig * gg
            h = og * np.tanh(c)
            state[s] = np.concatenate([h, c, ig, fg, gg, og], 1)
            sd = h @ w_out + b_out
            x = x + rd * sd.reshape(n, 1)
            trace[s + 1] = x
    return x.copy(), trace, state


def march_backward(views, tables, w_hh, w_out, rd, trace, state, grad_world, n_per_scene, steps, pos_grad,
                   dtype=np.float64, scatter=True):
    """avr_raymarch_bwd on the same inputs (the saved trace and state; the forward is not re-run), in dtype.
    Returns d_tables (n_scenes, H*W, 64), d_grads (1105: dW_hh 64 x 16, db 64, dw_out 16, db_out 1), S_tables and
    S_grads (per element, the sum of the absolute values of the terms added into it: for a table entry
    sum |w dg|), count (n_scenes, H*W: contributions with a non-zero weight per texel; every row of a texel gets
    the same ones), max_dg (max |dg| over finite values) and dh_pre (steps, n, 16: dh before the clamp).
    scatter=False skips the table gradient (the generators only need dh_pre)."""
    T = np.dtype(dtype).type
    tables, w_hh, w_out, rd, trace, state, gw = (np.asarray(a).astype(T) for a in
                                                 (tables, w_hh, w_out, rd, trace, state, grad_world))
    n = rd.shape[0]
    n_scenes = len(views)
    w_out = w_out.reshape(HID)
    d_tables, S_tables = np.zeros(tables.shape, T), np.zeros(tables.shape, T)
    count = np.zeros(tables.shape[:2], np.int64)
    dW, SW = np.zeros((GATES, HID), T), np.zeros((GATES, HID), T)
    db, Sb = np.zeros(GATES, T), np.zeros(GATES, T)
    dwo, Swo = np.zeros(HID, T), np.zeros(HID, T)
    dbo, Sbo = T(0), T(0)
    dx = gw.reshape(n, 3).copy()
    dh_next, dc_next = np.zeros((n, HID), T), np.zeros((n, HID), T)
    dh_pre = np.zeros((steps, n, HID), T)
    max_dg = 0.0
    with np.errstate(all="ignore"):
        for s in range(steps - 1, -1, -1):
            st = state[s]
            h, c, ig, fg, gg, og = (st[:, q * HID:(q + 1) * HID] for q in range(6))
            if s > 0:
                h_prev, c_prev = state[s - 1][:, :HID], state[s - 1][:, HID:2 * HID]
            else:
                h_prev, c_prev = np.zeros((n, HID), T), np.zeros((n, HID), T)
            dsd = (rd[:, 0] * dx[:, 0] + rd[:, 1] * dx[:, 1]) + rd[:, 2] * dx[:, 2]
            terms = dsd.reshape(n, 1) * h
            dwo, Swo = dwo + terms.sum(0), Swo + np.abs(terms).sum(0)
            dbo, Sbo = dbo + dsd.sum(), Sbo + np.abs(dsd).sum()
            dh = w_out.reshape(1, HID) * dsd.reshape(n, 1) + dh_next
            dh_pre[s] = dh
            dh = np.clip(dh, T(-CLAMP), T(CLAMP))   # a NaN stays NaN, as torch.clamp keeps it
            tc = np.tanh(c)
            dc = dh * og * (T(1) - tc * tc) + dc_next
            dg = np.concatenate([dc * gg * ig * (T(1) - ig), dc * c_prev * fg * (T(1) - fg),
                                 dc * ig * (T(1) - gg * gg), dh * tc * og * (T(1) - og)], 1)
            dc_next = dc * fg
            db, Sb = db + dg.sum(0), Sb + np.abs(dg).sum(0)
            dh_next = dg @ w_hh
            terms = dg.reshape(n, GATES, 1) * h_prev.reshape(n, 1, HID)
            dW, SW = dW + terms.sum(0), SW + np.abs(terms).sum(0)
            fin = np.isfinite(dg)
            if fin.any():
                max_dg = max(max_dg, float(np.abs(dg[fin]).max()))
            for sc, view in enumerate(views):
                sl = slice(sc * n_per_scene, (sc + 1) * n_per_scene)
                L = lookup(view, trace[s][sl])
                tb, dgs = tables[sc], dg[sl]
                if scatter:
                    for q in range(4):
                        contrib = L.w[:, q:q + 1] * dgs
                        np.add.at(d_tables[sc], L.tex[:, q], contrib)
                        np.add.at(S_tables[sc], L.tex[:, q], np.abs(contrib))
                        np.add.at(count[sc], L.tex[:, q], (L.w[:, q] != 0).astype(np.int64))
                if pos_grad:
                    tnw, tne, tsw, tse = (tb[L.tex[:, q]] for q in range(4))
                    gix = (dgs * (L.wy0.reshape(-1, 1) * (tne - tnw) + L.wy1.reshape(-1, 1) * (tse - tsw))).sum(1)
                    giy = (dgs * (L.wx0.reshape(-1, 1) * (tsw - tnw) + L.wx1.reshape(-1, 1) * (tse - tne))).sum(1)
                    dxc = gix.reshape(-1, 1) * L.dix + giy.reshape(-1, 1) * L.diy
                    R = _view_terms(view, T)[0]
                    dx[sl] = dx[sl] + dxc @ R   # R^T dxc
    d_grads = np.concatenate([dW.ravel(), db, dwo, np.reshape(dbo, 1)])
    S_grads = np.concatenate([SW.ravel(), Sb, Swo, np.reshape(Sbo, 1)])
    assert d_grads.shape == (N_GRADS,) and n_scenes == tables.shape[0]
    return SimpleNamespace(d_tables=d_tables, d_grads=d_grads, S_tables=S_tables, S_grads=S_grads, count=count,
                           max_dg=max_dg, dh_pre=dh_pre)


def rel_S(got, ref, S):
    """max_i |got_i - ref_i| / S_i over the elements with S_i > 0 (0.0 if there are none)."""
    got, ref, S = (np.asarray(a, np.float64).ravel() for a in (got, ref, S))
    m = S > 0
    return float((np.abs(got[m] - ref[m]) / S[m]).max()) if m.any() else 0.0


# ---------------------------------------------------------------------------------------------- input generators
def _rot(a, b):
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    Ry = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]])
    Rx = np.array([[1, 0, 0], [0, cb, -sb], [0, sb, cb]])
    return Ry @ Rx


def make_views(n_scenes, H, W):
    """One view per scene, all different: a rotation about two axes (R differs from R^T), focal and principal
    point unequal in x and y, a non-square image."""
    views = []
    for sc in range(n_scenes):
        poses = np.concatenate([_rot(0.5 + 0.37 * sc, -0.4 + 0.29 * sc),
                                np.array([[0.11 + 0.07 * sc], [-0.06 - 0.05 * sc], [0.23 + 0.04 * sc]])], 1)
        views.append({"poses": poses.astype(np.float32),
                      "focal": np.array([45.0 + 2.0 * sc, 37.0 - 1.5 * sc], np.float32),
                      "c": np.array([19.25 + 0.5 * sc, 15.75 - 0.25 * sc], np.float32),
                      "image_shape": np.array([40.0, 30.0], np.float32),
                      "latent_scaling": np.array([2.0 * W / (W - 1) * 0.97, 2.0 * H / (H - 1) * 1.02], np.float32),
                      "H": H, "W": W})
    return views


def unproject(view, ixr, iyr, zc):
    """World points (float64) whose lookup under view has the unclipped texel coordinates (ixr, iyr) at camera
    depth zc: the projection of lookup() inverted."""
    R, t, f, c, scale = _view_terms(view, np.float64)
    H, W = view["H"], view["W"]
    u = 2.0 * ixr / ((W - 1) * scale[0])
    v = 2.0 * iyr / ((H - 1) * scale[1])
    xc = np.stack([-(u - c[0]) / f[0] * zc, -(v - c[1]) / f[1] * zc, zc], 1)
    return (xc - t) @ R   # R^T (xc - t)


def _coord(rng, n, m, low=0.09, high=0.18, inside=None, margin=0.0):
    """Texel coordinates along an axis of m + 1 texels: a share `low` clipped below 0, `high` clipped above m (where
    X1 / Y1 saturate on the last row or column), the rest inside, at least `margin` from the texel centres."""
    kind = rng.random(n)
    lo, hi = inside if inside is not None else (0.0, float(m))
    ins = rng.uniform(lo, hi, n)
    ins = np.floor(ins) + margin + (ins - np.floor(ins)) * (1 - 2 * margin)
    return np.where(kind < low, rng.uniform(-1.5, -0.1, n), np.where(kind < low + high,
                                                                    rng.uniform(m + 0.1, m + 1.5, n), ins))


def _params(rng, min_w_out=0.0):
    w_hh = rng.uniform(-0.25, 0.25, (GATES, HID))
    b_ih, b_hh = rng.uniform(-0.2, 0.2, GATES), rng.uniform(-0.2, 0.2, GATES)
    b_ih[HID:2 * HID] += 1.0   # forget-gate bias, as the renderers initialise it
    w_out, b_out = rng.uniform(min_w_out, 0.25, HID) * rng.choice([-1.0, 1.0], HID), np.array([0.03])
    return [a.astype(np.float32) for a in (w_hh, b_ih, b_hh, w_out, b_out)]


def coords_ok(ixr, iyr, H, W):
    """Per lookup: no coordinate within TIE of a clip edge, none inside the map within TIE of an integer."""
    ok = True
    for v, m in ((ixr, W - 1), (iyr, H - 1)):
        v = np.asarray(v, np.float64)
        edge = (np.abs(v) > TIE) & (np.abs(v - m) > TIE)
        inside = (v > 0) & (v < m)
        ok = ok & edge & (~inside | (np.abs(v - np.rint(v)) > TIE))
    return ok


def dh_ok(dh_pre):
    """Per (step, ray, unit): the pre-clamp |dh| not within TIE relative of the clamp."""
    return np.abs(np.abs(np.asarray(dh_pre, np.float64)) - CLAMP) > TIE * CLAMP


def case_lookups(case, trace):
    """Unclipped (ixr, iyr), each (steps, n), of every lookup of a case along trace (float64)."""
    ixr, iyr = np.empty((case.steps, case.n)), np.empty((case.steps, case.n))
    for s in range(case.steps):
        for sc, view in enumerate(case.views):
            sl = slice(sc * case.n_per_scene, (sc + 1) * case.n_per_scene)
            L = lookup(view, np.asarray(trace[s][sl], np.float64))
            ixr[s, sl], iyr[s, sl] = L.ixr, L.iyr
    return ixr, iyr


def _case(views, tables, P, H, W, n_per_scene, steps, **arrays):
    c = SimpleNamespace(views=views, tables=tables, w_hh=P[0], b_ih=P[1], b_hh=P[2], w_out=P[3], b_out=P[4],
                        H=H, W=W, n_scenes=len(views), n_per_scene=n_per_scene, n=len(views) * n_per_scene,
                        steps=steps, **arrays)
    for a in vars(c).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)   # shared between tests: left unchanged
    return c


def forward(case, dtype=np.float64):
    return march_forward(case.views, case.tables, case.w_hh, case.b_ih, case.b_hh, case.w_out, case.b_out, case.ro,
                         case.rd, case.d0, case.n_per_scene, case.steps, dtype)


def backward(case, trace, state, grad_world, pos_grad, dtype=np.float64, scatter=True):
    return march_backward(case.views, case.tables, case.w_hh, case.w_out, case.rd, trace, state, grad_world,
                          case.n_per_scene, case.steps, pos_grad, dtype, scatter)


def _keep(ok_rays, n_per_scene, what):
    idx = np.flatnonzero(ok_rays)
    assert len(idx) >= n_per_scene, f"{what}: only {len(idx)} of {len(ok_rays)} candidate rays without a near-tie"
    return idx[:n_per_scene]


GW_SCALE = 60.0   # |grad_world| large enough that part of the h gradients exceed the clamp


@functools.lru_cache(maxsize=None)
def forward_case(H, W, n_scenes, n_per_scene, steps, seed=0):
    """Inputs of avr_raymarch_train (and, with grad_world, of the backward fed from its state): rays whose start
    points are placed at chosen texel coordinates (part of them clipped in x / y, part on the last row / column),
    marching along random directions."""
    rng = np.random.default_rng([seed, H, W, n_scenes, n_per_scene, steps])
    views = make_views(n_scenes, H, W)
    tables = (0.5 * rng.standard_normal((n_scenes, H * W, GATES))).astype(np.float32)
    P = _params(rng)
    m = 3 * n_per_scene + 24
    ro, rd, d0, gw = [], [], [], []
    for sc, view in enumerate(views):
        start = unproject(view, _coord(rng, m, W - 1), _coord(rng, m, H - 1), rng.uniform(0.8, 1.6, m))
        d = rng.standard_normal((m, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        dist = rng.uniform(0.5, 1.0, m)
        cand = _case([view], tables[sc:sc + 1], P, H, W, m, steps, ro=(start - d * dist[:, None]).astype(np.float32),
                     rd=d.astype(np.float32), d0=dist.astype(np.float32),
                     gw=(GW_SCALE * rng.standard_normal((m, 3))).astype(np.float32))
        _, trace, state = forward(cand)
        ok = coords_ok(*case_lookups(cand, trace), H, W).all(0)
        for pos_grad in (0, 1):
            ok &= dh_ok(backward(cand, trace, state, cand.gw, pos_grad, scatter=False).dh_pre).all((0, 2))
        keep = _keep(ok, n_per_scene, "forward_case")
        for lst, a in ((ro, cand.ro), (rd, cand.rd), (d0, cand.d0), (gw, cand.gw)):
            lst.append(a[keep])
    return _case(views, tables, P, H, W, n_per_scene, steps, ro=np.concatenate(ro), rd=np.concatenate(rd),
                 d0=np.concatenate(d0), gw=np.concatenate(gw))


def _synthetic_state(rng, steps, m, away=0.0):
    """away > 0 keeps |g| and |c| at least that far from 0 (no gate gradient is then tiny by itself)."""
    ig, fg, og = (rng.uniform(0.02, 0.98, (steps, m, HID)) for _ in range(3))
    gg = rng.uniform(away, 0.98, (steps, m, HID)) * rng.choice([-1.0, 1.0], (steps, m, HID))
    c = rng.uniform(away, 2.0, (steps, m, HID)) * rng.choice([-1.0, 1.0], (steps, m, HID))
    return np.concatenate([og * np.tanh(c), c, ig, fg, gg, og], 2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def synthetic_case(H, W, n_scenes, n_per_scene, steps, seed=0):
    """Inputs of avr_raymarch_bwd alone: gates drawn in (0, 1) / (-1, 1), c in (-2, 2), every step's trace point
    placed at a chosen texel coordinate (projection inverted in float64, rounded to fp32)."""
    rng = np.random.default_rng([seed, 1, H, W, n_scenes, n_per_scene, steps])
    views = make_views(n_scenes, H, W)
    tables = (0.5 * rng.standard_normal((n_scenes, H * W, GATES))).astype(np.float32)
    P = _params(rng)
    m = 3 * n_per_scene + 24
    rd, gw, trace, state = [], [], [], []
    for sc, view in enumerate(views):
        pts = np.stack([unproject(view, _coord(rng, m, W - 1), _coord(rng, m, H - 1), rng.uniform(0.8, 1.6, m))
                        for _ in range(steps + 1)]).astype(np.float32)
        d = rng.standard_normal((m, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        cand = _case([view], tables[sc:sc + 1], P, H, W, m, steps, rd=d.astype(np.float32),
                     gw=(GW_SCALE * rng.standard_normal((m, 3))).astype(np.float32), trace=pts,
                     state=_synthetic_state(rng, steps, m))
        ok = coords_ok(*case_lookups(cand, cand.trace), H, W).all(0)
        for pos_grad in (0, 1):
            ok &= dh_ok(backward(cand, cand.trace, cand.state, cand.gw, pos_grad, scatter=False).dh_pre).all((0, 2))
        keep = _keep(ok, n_per_scene, "synthetic_case")
        for lst, a in ((rd, cand.rd), (gw, cand.gw)):
            lst.append(a[keep])
        trace.append(cand.trace[:, keep])
        state.append(cand.state[:, keep])
    return _case(views, tables, P, H, W, n_per_scene, steps, rd=np.concatenate(rd), gw=np.concatenate(gw),
                 trace=np.concatenate(trace, 1), state=np.concatenate(state, 1))


GROUP = 64   # rays per group of two_group_case


@functools.lru_cache(maxsize=None)
def two_group_case(seed=0):
    """The fixed-point sums' dynamic range: one scene, a 5 x 7 map, 1 step, the clamp off. Group A (rays 0 .. 63)
    looks up texels of columns 0 .. 3, group B (rays 64 .. 127) of columns 4 .. 6, and B's grad_world is 2^-30 of
    the size of A's: B's table entries lie 30 bits below the call's largest gate gradient."""
    H, W, steps = 5, 7, 1
    rng = np.random.default_rng([seed, 2])
    views = make_views(1, H, W)
    tables = (0.5 * rng.standard_normal((1, H * W, GATES))).astype(np.float32)
    # no tiny out_layer weight, gate or cell value: every entry of group B then stays within a few bits of the
    # group's largest, and its relative error says how many bits the fixed-point grid left it
    P = _params(rng, min_w_out=0.1)
    m = 3 * GROUP
    parts = []
    for grp in range(2):
        ix = _coord(rng, m, W - 1, low=0.2, high=0.0, inside=(0.0, 3.0), margin=0.1) if grp == 0 else \
            _coord(rng, m, W - 1, low=0.0, high=0.3, inside=(4.0, 6.0), margin=0.1)
        pts = np.stack([unproject(views[0], ix, _coord(rng, m, H - 1, margin=0.1), rng.uniform(0.8, 1.6, m))] * 2)
        d = rng.standard_normal((m, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        g = 4.0 * rng.standard_normal((m, 3)) * (1.0 if grp == 0 else 2.0 ** -30)
        cand = _case(views, tables, P, H, W, m, steps, rd=d.astype(np.float32), gw=g.astype(np.float32),
                     trace=pts.astype(np.float32), state=_synthetic_state(rng, steps, m, away=0.25))
        keep = _keep(coords_ok(*case_lookups(cand, cand.trace), H, W).all(0), GROUP, "two_group_case")
        parts.append((cand.rd[keep], cand.gw[keep], cand.trace[:, keep], cand.state[:, keep]))
    rd, gw, trace, state = (np.concatenate([parts[0][i], parts[1][i]], 0 if i < 2 else 1) for i in range(4))
    return _case(views, tables, P, H, W, 2 * GROUP, steps, rd=rd, gw=gw, trace=trace, state=state)


@functools.lru_cache(maxsize=None)
def saturation_case(n, seed=0):
    """n identical rays at one texel centre (the last texel, reached by clipping both coordinates: weights exactly
    1, 0, 0, 0), identical state and grad_world, 1 step: the texel's entries are n * dg."""
    H, W, steps = 5, 7, 1
    rng = np.random.default_rng([seed, 3])
    views = make_views(1, H, W)
    tables = (0.5 * rng.standard_normal((1, H * W, GATES))).astype(np.float32)
    P = _params(rng)
    pt = unproject(views[0], np.array([W - 1 + 0.5]), np.array([H - 1 + 0.5]), np.array([1.1])).astype(np.float32)
    d = np.array([[0.48, -0.6, 0.64]])
    rep = lambda a: np.repeat(a, n, axis=-2)  # noqa: E731
    return _case(views, tables, P, H, W, n, steps, rd=rep(d.astype(np.float32)),
                 gw=rep(np.array([[3.0, 2.0, 5.0]], np.float32)), trace=rep(np.stack([pt, pt])),
                 state=rep(_synthetic_state(rng, steps, 1)))


def cbits_of(steps, n_rays):
    """avr_raymarch_bwd's count bits: the smallest cbits with 2^cbits >= 4 * steps * n_rays."""
    cbits = 0
    while (1 << cbits) < 4 * steps * n_rays:
        cbits += 1
    return cbits


def max_dg_exponent_ok(max_dg):
    """The frexp mantissa of max |dg| is not within TIE relative of a power of two: the kernels' fp32 max has the
    same exponent as the float64 one."""
    m, _ = np.frexp(max_dg)
    return 0.5 * (1 + TIE) < m < 1 - TIE
