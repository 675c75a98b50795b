"""The training-mode BatchNorm kernels (csrc/bn_train.hip), one by one, against tests/bn_ref.py (float64 numpy,
itself held to torch float64 by tests/test_bn_ref_cpu.py):

A. avr_bn_stats / avr_bn_grad_stats from synthetic per-workgroup partials, at row counts chosen by the depth of the
   two-stage fold (up to train.py's 163,840 rows: 2,560 partials, 160 fold rows) and at mean / std up to 4096.
B. avr_bn_grad_rows at row counts around its 16-row blocks.
C. avr_bn_layer_run alone with statistics vectors that are test inputs: the AVR_BN_RELU and AVR_BN_GRAD prologues,
   the per-workgroup partials, operand_out / operand_max, out_max.

Every bar is a count of fp32 roundings (2^-24 each, with a margin of 2) or the error of torch's fp32 GEMM on the same
operand; none is a measurement of the kernels. Each test prints its worst error next to its bar
(profiles/bn_kernel_errors.txt keeps one run's lines)."""
import functools

import numpy as np
import pytest
import torch

import bn_ref
from test_gpu_train_bn import _bn_net

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
F32 = torch.float32
U = 2.0 ** -24                      # one fp32 rounding, relative
EPS = float(np.float32(1e-5))       # BatchNorm1d's eps as the C float the kernel receives
POISON = 0x7FC0BEEF                 # a quiet NaN no kernel produces
SIGMA = 0.37


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _poisoned(*shape):
    return torch.full(shape, POISON, device=DEV, dtype=torch.int32).view(F32)


def _untouched(t):
    return bool((t.view(torch.int32) == POISON).all())


def _bits(x):
    """The uint32 bits of a non-negative float as the int32 word a max |.| buffer holds."""
    return int(np.float32(x).view(np.int32))


def _max_word(prefill=0.0):
    return torch.full((1,), _bits(prefill), device=DEV, dtype=torch.int32)


def _call(name, *args):
    from avr._lib import call
    call(name, *args)


def _p(t):
    from avr._lib import ptr
    return ptr(t)


def _stream():
    from avr._lib import stream_of
    return stream_of(torch.empty(1, device=DEV))


def _partial_buffer(M, C, p0, p1):
    """An avr_bn_partial_floats buffer holding the (nwg, 2, C) partials, NaN where nothing was written, with one
    more fold row (2 C doubles) of NaN behind it: a fold that reads one row too many reads NaN, within the buffer."""
    from avr._lib import size_query
    n = size_query("avr_bn_partial_floats", M, C)
    nwg = bn_ref.n_groups(M)
    assert n >= nwg * 2 * C and p0.shape == p1.shape == (nwg, C)
    buf = torch.full((n + 4 * C,), float("nan"), device=DEV, dtype=F32)
    buf[:nwg * 2 * C] = _dev(np.stack([p0, p1], 1).reshape(-1))
    return buf


def _report(what, worst):
    """worst: {name: (error, bar)} with error <= bar checked by the caller; one line per quantity."""
    for k, (e, b) in worst.items():
        print(f"{what}: {k} worst error/bar {e:.3f} ({b})")


def _worst(worst, name, err, bar, note):
    """Fold max(err / bar) into worst[name]; err and bar are arrays (bar > 0) or scalars."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(np.asarray(bar) > 0, np.asarray(err) / np.asarray(bar), np.where(np.asarray(err) > 0, np.inf, 0.0))
    r = float(np.max(r)) if np.size(r) else 0.0
    worst[name] = (max(r, worst.get(name, (0.0, note))[0]), note)
    return r


# ------------------------------------------------------------------ A. finalize kernels from synthetic partials
# rows -> fold rows (16 partials each) met by fold_rows' 16 waves: 1 partial of 2 rows; a last workgroup of 1 row;
# 2 fold rows, ragged; 16 (one per wave); 17 (the two-row loop's bound is false, the tail is taken); 34 (one loop
# trip plus the tail); 160 (train.py's step: five loop trips per wave)
FOLD_M = [2, 65, 1025, 16 * 1024, 17 * 1024 - 63, 33 * 1024 + 1, 163840]
FOLD_COLS = [4, 96, 512]            # 96: one and a half 64-column blocks (the c < N guards)
KINDS = [0.0, 1.0, 256.0, 4096.0, "constant"]     # mean / std of the synthetic columns


def _forward_partials(rng, kind, nwg, C):
    if kind == "constant":
        return np.full((nwg, C), 1000.0, np.float32), np.zeros((nwg, C), np.float32)
    p0 = kind * SIGMA + (SIGMA / 8) * rng.standard_normal((nwg, C))
    p1 = np.maximum(64 * SIGMA ** 2 * (1 + 0.2 * rng.standard_normal((nwg, C))), 0.0)
    return p0.astype(np.float32), p1.astype(np.float32)


@pytest.mark.parametrize("C", FOLD_COLS)
@pytest.mark.parametrize("M", FOLD_M)
def test_bn_stats_from_synthetic_partials(M, C):
    """avr_bn_stats: mu within one fp32 rounding (+ the fp64 fold's own error), invstd within one fp32 rounding plus
    the fp64 combine's worst-case cancellation, scale = gamma * invstd bit for bit, the running statistics as
    momentum * new + (1 - momentum) * old within four fp32 roundings, nothing written past the vectors' ends or
    through NULL running pointers."""
    rng = np.random.default_rng(1000 * C + M)
    T = bn_ref.n_groups(M)
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    old_m = rng.standard_normal(C).astype(np.float32)
    old_v = rng.uniform(0.5, 2.0, C).astype(np.float32)
    zeros = np.zeros(C)
    gamma_t, stream = _dev(gamma), _stream()
    worst = {}
    for kind in KINDS:
        p0, p1 = _forward_partials(rng, kind, T, C)
        # momentum 1 on zeros: the `new` of the running update (batch mean, unbiased variance)
        mu_r, is_r, _, new_m, new_v = bn_ref.stats_from_partials(p0, p1, M, gamma, EPS, 1.0, zeros, zeros)
        var_eps = 1.0 / is_r ** 2
        var = np.maximum(var_eps - EPS, 0.0)
        bar_mu = 2 * U * np.abs(mu_r) + T * 2.0 ** -50 * float(np.abs(p0).max())
        if kind == "constant":
            # integers throughout: the kernel's sums, mean and n * mean^2 are exact in fp64, so M2 = 0 exactly
            bar_is = np.full(C, 2 * U)
        else:
            bar_is = 2 * U + 2 * T * 2.0 ** -53 * (mu_r ** 2 + var) / var_eps
        part = _partial_buffer(M, C, p0, p1)
        for mom in (0.1, 1.0, 0.0, None):
            out = _poisoned(3, C + 8)
            rm, rv = (_dev(old_m), _dev(old_v)) if mom is not None else (None, None)
            m32 = float(np.float32(mom or 0.0))
            _call("avr_bn_stats", _p(part), M, C, _p(gamma_t), EPS, m32, _p(rm), _p(rv), _p(out[0]), _p(out[1]),
                  _p(out[2]), stream)
            mu, istd, scale = (_np(out[i, :C]) for i in range(3))
            assert _untouched(out[:, C:]), "wrote past mu / invstd / scale"
            e = _worst(worst, "mu", np.abs(mu.astype(np.float64) - mu_r), bar_mu, "2^-23 |ref| + T 2^-50 max|p0|")
            assert e <= 1.0, (kind, mom, "mu", e)
            e = _worst(worst, "invstd", np.abs(istd.astype(np.float64) / is_r - 1), bar_is,
                       "2^-23 + 2 T 2^-53 (mean^2 + var) / (var + eps)")
            assert e <= 1.0, (kind, mom, "invstd", e)
            assert np.array_equal(scale, gamma * istd), (kind, mom, "scale != gamma * invstd of the kernel's invstd")
            if mom is None:
                continue
            for name, new, old, got in (("running_mean", new_m, old_m, _np(rm)), ("running_var", new_v, old_v, _np(rv))):
                t1, t2 = m32 * new, (1.0 - m32) * old.astype(np.float64)
                e = _worst(worst, name, np.abs(got.astype(np.float64) - (t1 + t2)), 4 * U * (np.abs(t1) + np.abs(t2)),
                           "2^-22 (|momentum new| + |(1 - momentum) old|)")
                assert e <= 1.0, (kind, mom, name, e)
    _report(f"avr_bn_stats M={M} C={C} ({T} partials)", worst)


@pytest.mark.parametrize("C", FOLD_COLS)
@pytest.mark.parametrize("M", FOLD_M)
def test_bn_grad_stats_from_synthetic_partials(M, C):
    """avr_bn_grad_stats: m1 / m2 within one fp32 rounding of sum |p| / M, dgamma / dbeta ADDED to a non-zero
    prefill (bn_0 is applied twice per block: both applications accumulate), coef = gamma * invstd bit for bit."""
    rng = np.random.default_rng(2000 * C + M)
    T = bn_ref.n_groups(M)
    p0, p1 = ((rng.choice([-1.0, 1.0], (T, C)) * 2.0 ** rng.uniform(-20, 10, (T, C))).astype(np.float32)
              for _ in range(2))
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    istd = rng.uniform(0.5, 2.0, C).astype(np.float32)
    dg0 = (rng.standard_normal(C) * 100).astype(np.float32)
    db0 = (rng.standard_normal(C) * 100 + 3).astype(np.float32)
    _, m1_r, m2_r, dg_r, db_r = bn_ref.grad_stats_from_partials(p0, p1, M, gamma, istd, dg0, db0)
    out = _poisoned(3, C + 8)
    dg, db, gamma_t, istd_t, part = _dev(dg0), _dev(db0), _dev(gamma), _dev(istd), _partial_buffer(M, C, p0, p1)
    _call("avr_bn_grad_stats", _p(part), M, C, _p(gamma_t), _p(istd_t), _p(out[0]), _p(out[1]), _p(out[2]), _p(dg),
          _p(db), _stream())
    assert _untouched(out[:, C:]), "wrote past coef / m1 / m2"
    assert np.array_equal(_np(out[0, :C]), gamma * istd), "coef != gamma * invstd"
    worst = {}
    s0, s1 = np.abs(p0.astype(np.float64)).sum(0), np.abs(p1.astype(np.float64)).sum(0)
    for name, got, ref, bar in (("m1", _np(out[1, :C]), m1_r, 2 * U * s0 / M), ("m2", _np(out[2, :C]), m2_r, 2 * U * s1 / M),
                                ("dbeta", _np(db), db_r, 2 * U * (np.abs(db0) + np.abs(db_r - db0))),
                                ("dgamma", _np(dg), dg_r, 2 * U * (np.abs(dg0) + np.abs(dg_r - dg0)))):
        e = _worst(worst, name, np.abs(got.astype(np.float64) - ref), bar,
                   "2^-23 sum|p| / M" if name[0] == "m" else "2^-23 (|prefill| + |sum|)")
        assert e <= 1.0, (name, e)
    _report(f"avr_bn_grad_stats M={M} C={C} ({T} partials)", worst)


# ------------------------------------------------------------------ B. avr_bn_grad_rows
def _grad_inputs(rng, M, C, ratios, m2_max, res):
    """g, pre, (res), coef, m1, m2, mu, invstd as fp32 arrays; column c has mean / std = ratios[c % len]."""
    r = np.array([ratios[c % len(ratios)] for c in range(C)])
    std = rng.uniform(0.5, 2.0, C)
    d = dict(g=3 * rng.standard_normal((M, C)), pre=std * (r + rng.standard_normal((M, C))),
             res=rng.standard_normal((M, C)) * 2 if res else None,
             coef=rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C), m1=rng.standard_normal(C),
             m2=rng.uniform(-m2_max, m2_max, C), mu=std * r, invstd=1.0 / std)
    return {k: None if v is None else v.astype(np.float32) for k, v in d.items()}


def _grad_bar(d):
    """Four fp32 roundings with a 2x margin of coef * (g - m1 - xhat * m2), one more of res."""
    f = {k: None if v is None else v.astype(np.float64) for k, v in d.items()}
    xhat = (f["pre"] - f["mu"]) * f["invstd"]
    bar = 8 * U * np.abs(f["coef"]) * (np.abs(f["g"]) + np.abs(f["m1"]) + np.abs(xhat * f["m2"]))
    return bar if f["res"] is None else bar + 2 * U * np.abs(f["res"])


@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("C", [4, 260, 512])          # 260: 65 groups of 4 -- a second column block with one live group
@pytest.mark.parametrize("M", [1, 15, 16, 17, 63, 65, 1000])
def test_bn_grad_rows_vs_float64(M, C, res):
    """avr_bn_grad_rows element by element, nothing stored at or past n_rows, out_max NULL / kept where larger /
    exactly max |out| of the stored rows."""
    rng = np.random.default_rng(3000 * C + 2 * M + res)
    d = _grad_inputs(rng, M, C, (0.0, 300.0), 10.0, res)
    ref = bn_ref.grad_rows(d["g"], d["pre"], d["res"], d["coef"], d["m1"], d["m2"], d["mu"], d["invstd"])
    bar = _grad_bar(d)
    t = {k: None if v is None else _dev(v) for k, v in d.items()}
    worst = {}
    first = None
    for prefill in (None, 1e30, 0.0):
        word = None if prefill is None else _max_word(prefill)
        out = _poisoned(M + 3, C)
        _call("avr_bn_grad_rows", M, C, _p(t["g"]), _p(t["pre"]), _p(t["res"]), _p(t["coef"]), _p(t["m1"]), _p(t["m2"]),
              _p(t["mu"]), _p(t["invstd"]), _p(out), _p(word), _stream())
        assert _untouched(out[M:]), "rows at or past n_rows were written"
        got = _np(out[:M])
        e = _worst(worst, "out", np.abs(got.astype(np.float64) - ref), bar,
                   "2^-21 |coef| (|g| + |m1| + |xhat m2|) + 2^-23 |res|")
        assert e <= 1.0, e
        first = got if first is None else first
        assert np.array_equal(got, first), "out depends on out_max"
        if word is not None:   # a larger value survives; from 0 it is exactly max |out| of the rows just stored
            assert int(word.item()) == max(_bits(prefill), _bits(np.abs(got).max())), (prefill, int(word.item()))
    _report(f"avr_bn_grad_rows M={M} C={C} res={res}", worst)


# ------------------------------------------------------------------ C. avr_bn_layer_run with real statistics
CYCLE = [(0.0, 1.0), (8.0, 1e-3), (-8.0, 1.0), (300.0, 30.0)]     # (mean, std) of column c % 4
LAYER_M = [1, 63, 64, 65, 200]
LAYER_H = [64, 128, 256, 512]
N_BLOCKS = 2


@functools.lru_cache(maxsize=None)
def _layer_net(H):
    """A training-mode BatchNorm net of width H and what avr.bn_train takes from it: the forward blob packed
    without eval-BN folding, its dims, the backward blob."""
    from avr import _lib
    net = _bn_net(H, N_BLOCKS)
    fused = net.fused()
    entry = fused.packed(True, bn_fold=False)
    dims = entry.dims.with_precision(_lib.FIELD_X3)
    return net, entry, dims, fused.packed_bwd(True, entry)


def _layer(net, which):
    """(header index, nn.Linear) of fc_0[0] or fc_1[last]."""
    blocks = net.mlp_coarse.blocks
    return (2, blocks[0].fc_0) if which == "fc_0[0]" else (3 + 2 * (N_BLOCKS - 1), blocks[N_BLOCKS - 1].fc_1)


def _bn_rows(rng, M, H, dead=None):
    """Pre-BN rows (M, H) whose columns cycle through CYCLE, with the statistics vectors to match (inputs of the test,
    not kernel outputs): mu, invstd, scale = gamma * invstd, shift. No element's (x - mu) * scale + shift is within
    0.02 of the relu threshold before the rows are rounded to fp32; rows `dead` are all below it."""
    mean = np.array([CYCLE[c % 4][0] for c in range(H)])
    std = np.array([CYCLE[c % 4][1] for c in range(H)])
    gamma = rng.uniform(0.5, 1.5, H)
    beta = rng.uniform(0.1, 0.3, H) * rng.choice([-1.0, 1.0], H)
    xhat = rng.standard_normal((M, H))
    if dead is not None:
        xhat[dead] = -(np.abs(xhat[dead]) + 1.0)          # gamma >= 0.5 > beta: every value below the threshold
    z = gamma * xhat + beta
    xhat = np.where(np.abs(z) < 0.02, xhat + np.where(z >= 0, 0.04, -0.04) / gamma, xhat)
    rows = (mean + std * xhat).astype(np.float32)
    mu, invstd = mean.astype(np.float32), (1.0 / std).astype(np.float32)
    st = dict(mu=mu, invstd=invstd, scale=gamma.astype(np.float32) * invstd, shift=beta.astype(np.float32))
    return rows, st


def _check_masks(rows, st):
    """The two conditions the float64 reference must meet: no masked element within 1e-3 of the threshold (no mask
    can flip on rounding), at least a quarter of the masks on and a quarter off. -> the masks."""
    z = bn_ref.bn_pre_relu(rows, st["mu"], st["scale"], st["shift"])
    assert float(np.abs(z).min()) >= 1e-3, float(np.abs(z).min())
    on = float((z > 0).mean())
    assert 0.25 <= on <= 0.75, on
    return z > 0


def _gemm_errors(out_k, ref, out_t):
    s = float(np.abs(ref).max()) or 1.0
    return (float(np.abs(out_k.astype(np.float64) - ref).max()) / s,
            float(np.abs(_np(out_t).astype(np.float64) - ref).max()) / s)


def _run(dims, **kw):
    from avr import train_common as tc
    tc.run_layer(dims, tc.bn_layer(**kw), _stream())


@pytest.mark.parametrize("M", LAYER_M)
@pytest.mark.parametrize("which", ["fc_0[0]", "fc_1[last]"])
@pytest.mark.parametrize("H", LAYER_H)
def test_bn_layer_forward_relu_prologue(H, which, M):
    """AVR_BN_FWD with the AVR_BN_RELU prologue: operand_out, operand_max, out (+ add1), the per-workgroup (mean, M2)
    of the stored rows, and a workgroup whose operand is all <= 0 (split scale 1: out = bias (+ add1) bit for bit)."""
    from avr import _lib, train_common as tc
    net, entry, dims, _ = _layer_net(H)
    idx, lin = _layer(net, which)
    rng = np.random.default_rng(H * 1000 + M * 2 + idx)
    nwg = bn_ref.n_groups(M)
    dead = slice(64, min(128, M)) if nwg >= 2 else None     # workgroup 1 (M = 65: the 1-row last workgroup)
    rows, st = _bn_rows(rng, M, H, dead)
    _check_masks(rows, st)
    W, bias = _np(lin.weight), _np(lin.bias)
    add_np = rng.standard_normal((M, H)).astype(np.float32)
    src, bias_t = _dev(rows), lin.bias.detach().contiguous()
    tst = {k: _dev(v) for k, v in st.items()}
    op_ref = bn_ref.relu_operand(rows, st["mu"], st["scale"], st["shift"])
    d64 = rows.astype(np.float64) - st["mu"]
    bar_op = 4 * U * (np.abs(d64) * np.abs(st["scale"].astype(np.float64)) + np.abs(st["shift"]))
    worst = {}
    for add1, prefill in ((None, 0.0), (_dev(add_np), 1e30)):
        out, opnd = _poisoned(M + 2, H), _poisoned(M + 2, H)
        word = _max_word(prefill)
        part = tc.layer_partial(M, H, DEV)
        part.fill_(float("nan"))
        _run(dims, n_rows=M, mode=_lib.BN_FWD, prologue=_lib.BN_RELU, in_dim=H, in_valid=H, src=src, ld_src=H,
             in_mu=tst["mu"], in_scale=tst["scale"], in_shift=tst["shift"], operand_out=opnd, operand_max=word,
             blob=entry.packed, layer=idx, bias=bias_t, add1=add1, out=out, partial=part)
        assert _untouched(out[M:]) and _untouched(opnd[M:]), "rows past n_rows were written"
        op_k, out_k = _np(opnd[:M]), _np(out[:M])
        e = _worst(worst, "operand_out", np.abs(op_k.astype(np.float64) - op_ref), bar_op,
                   "2^-22 (|src - mu| |scale| + |shift|)")
        assert e <= 1.0, e
        assert not op_k[op_ref == 0].any(), "operand not exactly 0 under the relu"
        assert int(word.item()) == max(_bits(prefill), _bits(op_k.max())), "operand_max"
        # out from the operand the kernel stored, against torch's fp32 GEMM on the same operand
        a64 = None if add1 is None else add_np
        _, ref, _ = bn_ref.layer_fwd(None, W, bias, add1=a64, operand=op_k)
        out_t = torch.addmm(bias_t, opnd[:M], lin.weight.detach().t())
        eh, et = _gemm_errors(out_k, ref, out_t if add1 is None else out_t + add1)
        worst["out"] = (max(eh / max(2 * et, 2e-6), worst.get("out", (0.0, ""))[0]),
                        f"max(2 x torch fp32 addmm {et:.1e}, 2e-6) of max |out|; HIP {eh:.1e}")
        assert eh <= max(2 * et, 2e-6), (eh, et)
        if dead is not None:
            want = bias_t.expand(dead.stop - dead.start, H) if add1 is None else bias_t + add1[dead]
            assert torch.equal(out[dead], want), "all-dead workgroup: out != bias (+ add1) bit for bit"
        # partials of the kernel's stored rows (so the GEMM's error is not in them)
        pk = _np(part[:nwg * 2 * H]).reshape(nwg, 2, H)
        x64 = out_k.astype(np.float64)
        mean_r, _ = bn_ref.group_stats(x64)
        for w in range(nwg):
            x = x64[64 * w:64 * (w + 1)]
            e = _worst(worst, "partial mean", np.abs(pk[w, 0] - mean_r[w]), 14 * U * np.abs(x).mean(0),
                       "2 * 7 * 2^-24 mean|x|")
            assert e <= 1.0, (w, e)
            m2_r = ((x - pk[w, 0].astype(np.float64)) ** 2).sum(0)      # about the kernel's own mean
            ulp = np.spacing(np.abs(out_k[64 * w:64 * (w + 1)]).max(0)).astype(np.float64)
            e = _worst(worst, "partial M2", np.abs(pk[w, 1] - m2_r), 20 * U * m2_r + 64 * ulp ** 2,
                       "2 * 10 * 2^-24 M2 + 64 ulp(|x|max)^2")
            assert e <= 1.0, (w, e)
        if M == 1:
            assert np.array_equal(pk[0, 0], out_k[0]) and not pk[0, 1].any(), "one row: mean = the row, M2 = 0"
    _report(f"avr_bn_layer_run FWD/RELU H={H} {which} M={M}", worst)


@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("M", LAYER_M)
@pytest.mark.parametrize("which", ["fc_0[0]", "fc_1[last]"])
@pytest.mark.parametrize("H", LAYER_H)
def test_bn_layer_backward_grad_prologue(H, which, M, res):
    """AVR_BN_BWD with the AVR_BN_GRAD prologue: operand_out, out = mask * (W^T . op) (+ add1) with exact zeros under
    the mask, the per-workgroup (sum gp, sum gp * xhat) of the stored rows, out_max over the stored rows only."""
    from avr import _lib, train_common as tc
    net, entry, dims, bwd = _layer_net(H)
    idx, lin = _layer(net, which)
    rng = np.random.default_rng(H * 1000 + M * 4 + idx * 2 + res + 7)
    nwg = bn_ref.n_groups(M)
    # the operand: BatchNorm backward of g at the statistics `si` of src_pre
    src_pre, si = _bn_rows(rng, M, H)
    d = dict(g=rng.standard_normal((M, H)).astype(np.float32), pre=src_pre,
             res=rng.standard_normal((M, H)).astype(np.float32) if res else None, coef=si["scale"],
             m1=(0.1 * rng.standard_normal(H)).astype(np.float32), m2=rng.uniform(-1, 1, H).astype(np.float32),
             mu=si["mu"], invstd=si["invstd"])
    op_ref = bn_ref.grad_rows(d["g"], d["pre"], d["res"], d["coef"], d["m1"], d["m2"], d["mu"], d["invstd"])
    bar_op = _grad_bar(d)
    # the relu mask: of the layer input's pre-BN rows at the statistics `so`
    pre_rows, so = _bn_rows(rng, M, H)
    mask = _check_masks(pre_rows, so)
    W = _np(lin.weight)
    t = {k: None if v is None else _dev(v) for k, v in d.items()}
    tso = {k: _dev(v) for k, v in so.items()}
    pre_t = _dev(pre_rows)
    xhat = (pre_rows.astype(np.float64) - so["mu"]) * so["invstd"].astype(np.float64)
    m0 = 64 * (nwg - 1)
    worst = {}
    add_last = gp_first = big = None
    # third run: a residual gradient add1 whose row m0 would win out_max through a dead row of a partial last tile
    for prefill, with_add in ((0.0, False), (1e30, False), (0.0, True)):
        add1 = add_last if with_add else None
        out, opnd = _poisoned(M + 2, H), _poisoned(M + 2, H)
        word, opword = _max_word(prefill), _max_word(prefill)
        part = tc.layer_partial(M, H, DEV)
        part.fill_(float("nan"))
        _run(dims, n_rows=M, mode=_lib.BN_BWD, prologue=_lib.BN_GRAD, in_dim=H, in_valid=H, src=t["g"], ld_src=H,
             src_pre=t["pre"], src_res=t["res"], in_mu=t["mu"], in_invstd=t["invstd"], in_scale=t["coef"],
             in_m1=t["m1"], in_m2=t["m2"], operand_out=opnd, operand_max=opword, blob=bwd, layer=idx, add1=add1,
             out=out, pre_rows=pre_t, out_mu=tso["mu"], out_invstd=tso["invstd"], out_scale=tso["scale"],
             out_shift=tso["shift"], partial=part, out_max=word)
        assert _untouched(out[M:]) and _untouched(opnd[M:]), "rows past n_rows were written"
        op_k, out_k = _np(opnd[:M]), _np(out[:M])
        e = _worst(worst, "operand_out", np.abs(op_k.astype(np.float64) - op_ref), bar_op,
                   "2^-21 |scale| (|g| + |m1| + |xhat m2|) + 2^-23 |res|")
        assert e <= 1.0, e
        assert int(opword.item()) == max(_bits(prefill), _bits(np.abs(op_k).max())), "operand_max"
        assert int(word.item()) == max(_bits(prefill), _bits(np.abs(out_k).max())), "out_max: the stored rows' max"
        a64 = None if add1 is None else _np(add1)
        _, _, ref, _ = bn_ref.layer_bwd(None, W, pre_rows, (so["mu"], so["invstd"], so["scale"], so["shift"]),
                                        add1=a64, operand=op_k)
        out_t = (opnd[:M] @ lin.weight.detach()) * _dev(mask)
        eh, et = _gemm_errors(out_k, ref, out_t if add1 is None else out_t + add1)
        worst["out"] = (max(eh / max(2 * et, 2e-6), worst.get("out", (0.0, ""))[0]),
                        f"max(2 x torch fp32 GEMM {et:.1e}, 2e-6) of max |out|; HIP {eh:.1e}")
        assert eh <= max(2 * et, 2e-6), (eh, et)
        pk = _np(part[:nwg * 2 * H]).reshape(nwg, 2, H)
        if not with_add:
            assert not out_k[~mask].any(), "out not exactly 0 where the mask is off"
            gp = out_k.astype(np.float64)
            s1_r, s2_r = bn_ref.group_grad_sums(gp, pre_rows, so["mu"], so["invstd"])
            for w in range(nwg):
                sl = slice(64 * w, 64 * (w + 1))
                for k, name, ref_s, terms in ((0, "partial sum gp", s1_r, gp[sl]),
                                              (1, "partial sum gp xhat", s2_r, gp[sl] * xhat[sl])):
                    e = _worst(worst, name, np.abs(pk[w, k] - ref_s[w]), 16 * U * np.abs(terms).sum(0),
                               "2 * 8 * 2^-24 sum|terms|")
                    assert e <= 1.0, (w, name, e)
            if gp_first is None:
                # add1 of the last run: row m0 (the row the dead rows of a partial last tile load) larger than every
                # other stored |out| and opposed to gp, so that the stored rows stay below `big` and a dead row
                # entering out_max would raise it to `big`
                gp_first = pk.copy()
                big = 4.0 * float(np.abs(out_k).max()) + 8.0
                add_np = rng.standard_normal((M, H)).astype(np.float32)
                add_np[m0] = np.where(out_k[m0] > 0, -big, np.where(out_k[m0] < 0, big, 0.5))
                add_last = _dev(add_np)
        else:
            assert np.array_equal(pk, gp_first), "the partials are of gp alone, not of gp + add1"
            assert float(np.abs(out_k).max()) < big
    _report(f"avr_bn_layer_run BWD/GRAD H={H} {which} M={M} res={res}", worst)
