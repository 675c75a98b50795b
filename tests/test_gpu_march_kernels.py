"""The LSTM march's training kernels (csrc/raymarch.hip: avr_raymarch_train, avr_raymarch_bwd; avr_raymarch beside
them) called through avr._lib on arrays the test constructs, every output element against the float64 reference
of tests/march_ref.py on the same inputs. The yardstick is the same reference run in float32 (the kernels' number
format): a kernel may be at most twice as far from float64 as that run. Errors of the backward are measured per
element against S, the sum of the absolute values of the terms added into that element, so a wrong value in a
rarely visited texel or one W_hh row counts as much as one in the largest entry. The inputs' conditions (no
near-ties; the clamp, clipped coordinates and border texels covered) are asserted in tests/test_march_ref_cpu.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import march_ref as mr
from test_march_ref_cpu import FORWARD_CASES, SATURATION_RAYS, SYNTHETIC_CASES

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
FLOOR = 2.0 ** -22   # the final roundings, when the float32 run happens to be exact
_ids = lambda a: "x".join(map(str, a))  # noqa: E731


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a, np.float32), device=DEV)


def _views(case):
    from avr import _lib
    arr = (_lib.ViewDesc * case.n_scenes)()
    for v, view in zip(arr, case.views):
        v.poses[:] = [float(x) for x in view["poses"].ravel()]
        for name in ("focal", "c", "image_shape", "latent_scaling"):
            getattr(v, name)[:] = [float(x) for x in view[name]]
        v.latent_h, v.latent_w = view["H"], view["W"]
    return arr


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


def hip_forward(case):
    """avr_raymarch_train: world, trace, state as fp32 numpy arrays (outputs pre-filled with NaN)."""
    from avr import _lib
    n, steps = case.n, case.steps
    world, trace, state = _nan(n, 3), _nan(steps + 1, n, 3), _nan(max(steps, 1), n, mr.STATE)
    args = [_dev(a) for a in (case.tables, case.w_hh, case.b_ih, case.b_hh, case.w_out, case.b_out, case.ro,
                              case.rd, case.d0)]
    _lib.call("avr_raymarch_train", _views(case), case.n_scenes, *[_lib.ptr(t) for t in args], case.n_per_scene,
              steps, _lib.ptr(world), _lib.ptr(trace), _lib.ptr(state), _lib.stream_of(world))
    return world.cpu().numpy(), trace.cpu().numpy(), state[:steps].cpu().numpy()


def hip_inference_trace(case):
    """avr_raymarch on scene 0's rays: its trace."""
    from avr import _lib
    n, steps = case.n_per_scene, case.steps
    world, trace = _nan(n, 3), _nan(steps + 1, n, 3)
    args = [_dev(a) for a in (case.tables[0], case.w_hh, case.b_ih, case.b_hh, case.w_out, case.b_out, case.ro[:n],
                              case.rd[:n], case.d0[:n])]
    _lib.call("avr_raymarch", ctypes.byref(_views(case)[0]), *[_lib.ptr(t) for t in args], n, steps,
              _lib.ptr(world), None, _lib.ptr(trace), _lib.stream_of(world))
    assert np.array_equal(world.cpu().numpy(), trace[steps].cpu().numpy())
    return trace.cpu().numpy()


def hip_backward(case, trace, state, grad_world, pos_grad, steps=None):
    """avr_raymarch_bwd: d_tables, d_grads as fp32 numpy arrays. The outputs are pre-filled with NaN (they are
    written whole) and the scratch with a non-zero byte (the call clears what it needs)."""
    from avr import _lib
    steps = case.steps if steps is None else steps
    d_tables, d_grads = _nan(*case.tables.shape), _nan(mr.N_GRADS)
    nb = ctypes.c_int64(0)
    _lib.check(_lib.load().avr_raymarch_bwd_scratch_bytes(case.n, steps, case.tables.size, ctypes.byref(nb)),
               "avr_raymarch_bwd_scratch_bytes")
    scratch = torch.full((max(nb.value, 1),), 0xAB, device=DEV, dtype=torch.uint8)
    args = [_dev(a) for a in (case.tables, case.w_hh, case.w_out, case.rd, trace, state, grad_world)]
    _lib.call("avr_raymarch_bwd", _views(case), case.n_scenes, *[_lib.ptr(t) for t in args], case.n_per_scene,
              steps, pos_grad, _lib.ptr(d_tables), _lib.ptr(d_grads), _lib.ptr(scratch), scratch.numel(),
              _lib.stream_of(d_tables))
    return d_tables.cpu().numpy(), d_grads.cpu().numpy()


# ------------------------------------------------------------------------------------------------- 3a: forward
@functools.lru_cache(maxsize=None)
def _hip_forward_cached(args):
    out = hip_forward(mr.forward_case(*args))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _forward_refs(args):
    case = mr.forward_case(*args)
    return mr.forward(case), mr.forward(case, np.float32)


@functools.lru_cache(maxsize=None)
def _forward_yardstick(H, W, steps):
    """Worst |float32 run - float64 run| of world, trace and state over the forward cases of one latent size and
    step count. The cases share one generator and differ in the number of rays: the worst of a few hundred rays
    is a stable figure, the worst of one ray (96 state values) is luck, and a kernel is no more accurate on a
    launch of one ray. The bar is twice this."""
    worst = [0.0, 0.0, 0.0]
    for args in FORWARD_CASES:
        if (args[0], args[1], args[4]) == (H, W, steps):
            r64, r32 = _forward_refs(args)
            worst = [max(w, float(np.abs(a32.astype(np.float64) - a64).max())) for w, a32, a64 in
                     zip(worst, r32, r64)]
    return worst


@pytest.mark.parametrize("args", FORWARD_CASES, ids=_ids)
def test_train_forward_vs_float64(args):
    """avr_raymarch_train's world, trace and saved state, and avr_raymarch's trace on scene 0's rays, element by
    element against march_forward in float64; the bar is twice the float32 run's worst distance from float64
    (a few fp32 ulp at 1 step, amplified by the recurrence at 10)."""
    case = mr.forward_case(*args)
    got = _hip_forward_cached(args)
    ref = _forward_refs(args)[0]
    yard = _forward_yardstick(args[0], args[1], args[4])
    assert all(0 < y < 1e-3 for y in yard), yard
    errs = [float(np.abs(g.astype(np.float64) - r).max()) for g, r in zip(got, ref)]
    inf_trace = hip_inference_trace(case)
    err_inf = float(np.abs(inf_trace.astype(np.float64) - ref[1][:, :case.n_per_scene]).max())
    same = np.array_equal(inf_trace, got[1][:, :case.n_per_scene])
    print(f"\nforward {_ids(args)}: |HIP - f64| world {errs[0]:.2e} trace {errs[1]:.2e} state {errs[2]:.2e}; "
          f"float32 run {yard[0]:.2e} {yard[1]:.2e} {yard[2]:.2e}; inference trace {err_inf:.2e}, "
          f"bit-identical to the training trace: {same}")
    for name, e, y in zip(("world", "trace", "state"), errs, yard):
        assert e <= 2.0 * y, f"{name}: HIP {e:.3e} from float64, the float32 run {y:.3e}"
    assert err_inf <= 2.0 * yard[1], f"avr_raymarch trace: {err_inf:.3e} from float64, the float32 run {yard[1]:.3e}"


# ------------------------------------------------------------------------------------------------ 3b: backward
def _check_backward(tag, got, ref, f32, tables_mask=None):
    """Every output tensor of the backward: max |got - ref64| / S at most twice the float32 run's plus 2^-22, and
    exactly 0.0 where S is 0 (a texel no ray touched, W_hh's gradient of a 1-step march). tables_mask limits the
    table entries held to the bar (the zero check always covers all). Returns the measured metrics."""
    d_tables, d_grads = got
    tensors = [("d_tables", d_tables, ref.d_tables, f32.d_tables, ref.S_tables)]
    tensors += [(name, d_grads[sl], ref.d_grads[sl], f32.d_grads[sl], ref.S_grads[sl])
                for name, sl in mr.BLOCKS.items()]
    out, msgs = {}, []
    for name, g, r, y, S in tensors:
        zero = S == 0
        assert np.array_equal(g[zero], np.zeros_like(g[zero])), f"{tag} {name}: a value where nothing was added"
        if name == "d_tables" and tables_mask is not None:
            S = np.where(tables_mask, S, 0.0)
        m, m32 = mr.rel_S(g, r, S), mr.rel_S(y, r, S)
        out[name] = (m, m32)
        msgs.append(f"{name} {m:.2e} ({m32:.2e})")
    print(f"\nbackward {tag}: max |HIP - f64| / S (float32 run): " + ", ".join(msgs))
    for name, (m, m32) in out.items():
        assert m <= 2.0 * m32 + FLOOR, f"{tag} {name}: HIP {m:.3e} of S from float64, the float32 run {m32:.3e}"
    return out


@pytest.mark.parametrize("pos_grad", [1, 0])
@pytest.mark.parametrize("args", FORWARD_CASES, ids=_ids)
def test_backward_on_forward_state_vs_float64(args, pos_grad):
    """avr_raymarch_bwd fed with the trace and state avr_raymarch_train produced; the float64 reference consumes
    exactly those arrays."""
    case = mr.forward_case(*args)
    _, trace, state = _hip_forward_cached(args)
    got = hip_backward(case, trace, state, case.gw, pos_grad)
    ref = mr.backward(case, trace, state, case.gw, pos_grad)
    f32 = mr.backward(case, trace, state, case.gw, pos_grad, np.float32)
    _check_backward(f"forward-fed {_ids(args)} pos_grad={pos_grad}", got, ref, f32)


@pytest.mark.parametrize("pos_grad", [1, 0])
@pytest.mark.parametrize("args", SYNTHETIC_CASES, ids=_ids)
def test_backward_on_synthetic_state_vs_float64(args, pos_grad):
    """avr_raymarch_bwd on a state no forward produced (gates drawn in (0, 1) / (-1, 1), c in (-2, 2)) and trace
    points placed at chosen texel coordinates."""
    case = mr.synthetic_case(*args)
    got = hip_backward(case, case.trace, case.state, case.gw, pos_grad)
    ref = mr.backward(case, case.trace, case.state, case.gw, pos_grad)
    f32 = mr.backward(case, case.trace, case.state, case.gw, pos_grad, np.float32)
    _check_backward(f"synthetic {_ids(args)} pos_grad={pos_grad}", got, ref, f32)


# ------------------------------------------------------------------------------------- 3c: the fixed-point sums
def _fixed_point_bound(case, ref, f32, count=None):
    """Per table entry: n_i 2^(cbits + e - 63) + (3b's bar) S_i + 2^-24 |ref64_i|. The scale of the int64 sums is
    2^(62 - cbits - e) with e the frexp exponent of max |dg| and 2^cbits >= 4 steps n_rays contributions, so one
    contribution is rounded by at most half a grid step, 2^(cbits + e - 63); the conversion of the sum to fp32
    rounds once more (2^-24 |ref|); the fp32 term covers the error dg and w carry in."""
    cbits = mr.cbits_of(case.steps, case.n)
    e = int(np.frexp(ref.max_dg)[1])
    bar = 2.0 * mr.rel_S(f32.d_tables, ref.d_tables, ref.S_tables) + FLOOR
    count = ref.count if count is None else count
    return count[..., None] * 2.0 ** (cbits + e - 63) + bar * ref.S_tables + 2.0 ** -24 * np.abs(ref.d_tables), cbits


def test_fixed_point_dynamic_range():
    """Table entries 30 bits below the call's largest gate gradient (group B of two_group_case) meet the stated
    bound, and keep a relative accuracy: a scale wrong by many bits, or a flush to zero, fails."""
    case = mr.two_group_case()
    got = hip_backward(case, case.trace, case.state, case.gw, 1)
    ref = mr.backward(case, case.trace, case.state, case.gw, 1)
    f32 = mr.backward(case, case.trace, case.state, case.gw, 1, np.float32)
    colA = np.broadcast_to((np.arange(case.H * case.W) % case.W < 4)[None, :, None], ref.S_tables.shape)
    _check_backward("two groups (group A's entries)", got, ref, f32, tables_mask=colA)
    bound, cbits = _fixed_point_bound(case, ref, f32)
    B = ~colA & (ref.S_tables > 0)
    assert B.sum() >= 10 * mr.GATES // 2
    err = np.abs(got[0].astype(np.float64) - ref.d_tables)
    assert (err[B] <= bound[B]).all(), float((err[B] / bound[B]).max())
    rel = err[B] / ref.S_tables[B]
    implied = bound[B] / ref.S_tables[B]
    n_max = int(ref.count[0][(np.arange(case.H * case.W) % case.W) >= 4].max())
    print(f"\ntwo groups: group B (2^-30 of A) max |HIP - f64| / S = {rel.max():.3e} = 2^{np.log2(rel.max()):.1f}; "
          f"cbits {cbits}, at most {n_max} contributions per entry, n 2^(cbits - 33) = "
          f"2^{np.log2(n_max) + cbits - 33:.1f}; the bound implies at most 2^{np.log2(implied.max()):.1f}")
    assert (rel <= implied).all()
    assert rel.max() < 2.0 ** -10


@pytest.mark.parametrize("n", SATURATION_RAYS)
def test_fixed_point_saturation(n):
    """n same-sign contributions of the call's largest size into one entry (4 n = 2^12 and 2^12 + 4: cbits steps
    from 12 to 13): the sum is n dg within the bound -- no int64 wrap, no off-by-one in cbits."""
    case = mr.saturation_case(n)
    got = hip_backward(case, case.trace, case.state, case.gw, 1)
    ref = mr.backward(case, case.trace, case.state, case.gw, 1)
    f32 = mr.backward(case, case.trace, case.state, case.gw, 1, np.float32)
    bound, cbits = _fixed_point_bound(case, ref, f32)
    assert cbits == (12 if n == 1024 else 13)
    err = np.abs(got[0].astype(np.float64) - ref.d_tables)
    hit = ref.S_tables > 0
    assert hit.sum() == 3 * mr.HID and hit[0, -1].sum() == 3 * mr.HID
    print(f"\nsaturation n={n}: cbits {cbits}, max |HIP - n dg| / (n |dg|) = "
          f"{(err[hit] / ref.S_tables[hit]).max():.3e}; bound / (n |dg|) at most {(bound[hit] / ref.S_tables[hit]).max():.3e}")
    assert (err[hit] <= bound[hit]).all()
    # stricter than the bound's fp32 term, which the float32 run's sequential sum of n values inflates: the int64
    # sum is exact and every dg the same, so the entry is n * fp32(dg) up to the roundings above
    assert (err[hit] / ref.S_tables[hit]).max() < 2.0 ** -10
    assert not got[0][~hit].any()
    _check_backward(f"saturation n={n}", got, ref, f32)


# -------------------------------------------------------------------------------------- 3d: non-finite gradient
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_gradient(bad):
    """One group-A ray of two_group_case with a NaN (then +inf) grad_world: the entries its lookup touches are NaN,
    every other entry is what the call without that ray gives (group B's still within the fixed-point bound), and
    the parameter gradients are non-finite where the reference's sums are."""
    case = mr.two_group_case()
    # a ray whose direction has components of both signs, so that +inf in every component of grad_world gives
    # rd . grad_world = inf - inf = NaN (one sign would give inf, which the clamp turns into a finite 10)
    # -- and whose lookup is inside the map: four distinct texels, every weight non-zero
    LA = mr.lookup(case.views[0], case.trace[0][:mr.GROUP].astype(np.float64))
    ray = int(np.flatnonzero((case.rd[:mr.GROUP] > 0).any(1) & (case.rd[:mr.GROUP] < 0).any(1)
                             & (LA.w != 0).all(1))[0])
    gw_bad, gw_wo = case.gw.copy(), case.gw.copy()
    gw_bad[ray], gw_wo[ray] = bad, 0.0
    got = hip_backward(case, case.trace, case.state, gw_bad, 1)
    ref_with = mr.backward(case, case.trace, case.state, gw_bad, 1)
    ref = mr.backward(case, case.trace, case.state, gw_wo, 1)
    f32 = mr.backward(case, case.trace, case.state, gw_wo, 1, np.float32)
    L = mr.lookup(case.views[0], case.trace[0][ray:ray + 1].astype(np.float64))
    assert (L.w[0] != 0).all()
    touched = np.zeros(ref.S_tables.shape, bool)
    touched[0, L.tex[0]] = True
    assert np.isnan(ref_with.d_tables[touched]).all() and np.isfinite(ref_with.d_tables[~touched]).all()
    assert np.isnan(got[0][touched]).all()
    count = ref.count.copy()
    count[0, L.tex[0]] -= 1           # the zeroed ray adds nothing in the kernel's run
    bound, _ = _fixed_point_bound(case, ref, f32, count)
    rest = ~touched
    zero = rest & (ref.S_tables == 0)
    assert not got[0][zero].any()
    err = np.abs(got[0].astype(np.float64) - ref.d_tables)
    held = rest & (ref.S_tables > 0)
    assert np.isfinite(got[0][held]).all()
    assert (err[held] <= bound[held]).all(), float((err[held] / bound[held]).max())
    colB = np.broadcast_to((np.arange(case.H * case.W) % case.W >= 4)[None, :, None], held.shape)
    assert (held & colB).sum() >= 10 * mr.GATES // 2
    assert (err[held & colB] / ref.S_tables[held & colB]).max() < 2.0 ** -10
    finite_ref = np.isfinite(ref_with.d_grads)
    assert not finite_ref.all()
    assert np.array_equal(np.isfinite(got[1]), finite_ref)
    print(f"\nnon-finite ({bad}): {int(touched.sum())} entries NaN, {int(held.sum())} others within the bound "
          f"(worst {float((err[held] / bound[held]).max()):.2f} of it), {int((~finite_ref).sum())} of "
          f"{mr.N_GRADS} parameter gradients non-finite")


# ---------------------------------------------------------------------------------------------- 3e: zero steps
def test_backward_zero_steps_writes_zeros():
    """steps = 0: nothing was marched, every gradient is exactly zero (all scenes' tables, every d_grads value),
    written over whatever the buffers held."""
    case = mr.forward_case(5, 7, 3, 65, 1)
    _, trace, state = _hip_forward_cached((5, 7, 3, 65, 1))
    d_tables, d_grads = hip_backward(case, trace, state, case.gw, 1, steps=0)
    assert d_tables.shape == (3, 35, 64) and d_grads.shape == (mr.N_GRADS,)
    assert np.array_equal(d_tables, np.zeros_like(d_tables)) and np.array_equal(d_grads, np.zeros_like(d_grads))
