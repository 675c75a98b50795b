"""The fused field-training kernels -- avr_field_fwd_points_train, avr_field_bwd, avr_weight_grads on the maxima the
first two track -- called through the C ABI and compared layer by layer with tests/field_train_ref.py (float64 numpy,
itself held to torch float64 autograd by tests/test_field_train_ref_cpu.py, which also checks this file's inputs).

The method is *local*: every comparison takes the rows the kernels stored (act[l], G[l], z_feature, out) as the
operands of the float64 reference, so it spans one GEMM and no error compounds through the weights, and every element
is compared: ReLU and Softplus are 1-Lipschitz, so a pre-activation the kernel rounded to the other side of zero is
inside the bar, and the backward's relu masks are decided by the kernel's own stored activation (act > 0 exactly).
The lin_z term of the residual stream is the float64 bilinear blend of the *input* table rows with the corner weights
of oracle.avr_oracle.grid_sample_bilinear_border at the kernel's own stored xyz_rot (z_feature[:, :3]): IEEE fp32
adds, multiplies, divides and floors in bilinear_from_rot's order, which the kernel's uncontracted fadd / fmul / fdiv
reproduce bit for bit.

Nets: tests/test_gpu_train.py's _net, d_latent 64, an 8 x 8 map, 3 blocks, combine_layer 2 (block 2 has no lin_z),
three scenes with their own maps and poses. Rows: M per scene in {1, 63, 64, 65, 130} of one scene (a partial
workgroup, a full one, one row in a second, two full plus two rows) and 3 scenes x 65 (scene offsets that are no
multiple of 64, every scene ending in a one-row workgroup). Layouts: d_hidden 64 / 128 / 256 / 512, at 512 the four
(AVR_X3_SAVE_WAVES, AVR_X3_BWD_WAVES) pairs -- the 8-wave forward writes its relu masks in the 4-wave layout's words
(mask_words8) and both backward layouts read either -- and Softplus(1.5) at 64 and 512.

THE BARS. U = 2^-24, one fp32 rounding, relative. No bar is a measurement of the kernels.

The x3 product W.x ~ Wh.xh + Wh.xl + Wl.xh under power-of-two scales: hi = fp16(v s) leaves a residual of at most
2^-11 |v s|, lo = fp16 of that residual (exact in fp32) leaves 2^-11 of it: hi + lo holds an operand to 2^-22 = 4 U
relative (not U), and the dropped Wl.xl is at most 2^-11 2^-11 = 4 U of the term. A lo half below fp16's normal range
(2^-14 under a scale that puts the tensor's max in [2^13, 2^14)) is held to the subnormal spacing 2^-24 instead:
2^-37 of the tensor's max per element (`_tiny`). The MFMA chain adds 3 K / 32 times onto the fp32 accumulator, after a
32-term dot each (6 roundings if it is a binary tree of fp32 adds, and it is at least that precise): 3 K / 32 + 6 <= K
roundings of a partial sum that never exceeds sum |w x| (+ |the accumulator's start|) for every K >= 64 here, also if
the hardware truncates (2 U per step) -- the K of "(K + c) U".

Rigorous, elementwise: |kernel - reference| <= (K + c) U (|W| @ |x| + |b|) + _tiny (+ the store's rounding), with
  forward fc_0 (act[2b+1]), c = C_FC = 13: W split 4, x split 4, Wl.xl 4, the bias fma 1 (the rescale by 1 / S is a
    power of two; relu is exact; the stored fp32 act row IS the value that was split);
  residual stream (act[2b], act[2 nb]), c = C_STREAM = 23 per step: the 12 of the products, the lin_z bias folded into
    the layer's bias at pack time 1, the accumulator's start h r + b S (one fma) 1, the blend's 4 products and 4 adds
    into h 8, the fp32 rounding of the oracle function's result 1. The ingredient of a step includes |x_b|, the
    accumulator the GEMM adds onto, and the blend of |table rows|; K is 64 for lin_in (its K is padded to 64) and
    d_hidden for fc_1. The kernel's stream carries its error on, so block b's bar is the SUM of the steps' bars up to b;
  lin_out (out), c = C_OUT = 22: 12, the bias 1, the 8-wave layout's per-wave partial sums added in fp32 8, their
    rescale 1; the sigmoids pass a quarter of the raw error (max slope 1 / 4) plus 4 roundings of their own
    (expf, the add, the division, 1 spare) of a value <= 1; the relu passes it as it is;
  Softplus adds 1 to c (the rounding of beta x passes through a slope <= 1) and 10 U |y|: expf and log1pf at the
    2 ulp = 4 U of the OpenCL conformance bound HIP's device library is built to, a correctly rounded division 1, 1
    spare (log1p(exp(.)) has a relative condition number <= 1);
  backward GEMMs (G[2b]; the GEMM part of G[2b-1] and G[2 nb]), c = C_BWD = 8: W^T split 4, Wl.xl 4 -- the stored G row
    is (hi + lo) / s_x, the operand itself, so the x side has no error against the stored rows; the unscale is a power
    of two and the relu mask exact. Softplus slopes 1 - exp(-beta y) add 6 (beta y 1, expm1f 4, the product 1);
  the row store (RowSide: every G[l] but G[2 nb], which store_rows writes as the fp32 registers): (hi + lo) / s_x of the
    register value, 4 U |value| + 2^-37 of the layer's max;
  the residual adds G[2b+1] + (...): the kernel adds onto its REGISTER dx, the reference onto the stored row:
    4 U |G[2b+1]| + 2^-37 max, one rounding of the sum, and the store of the result;
  lin_out^T (G[2 nb - 1]), K = 4 fp32 fmas, c = C_LAST = 3: the three roundings of g (1 - y) y.

Tight, per layer: max |kernel - reference| <= TIGHT x max |torch fp32 of the same operands - reference| + floor,
TIGHT = 2 (tests/test_gpu_train.py _compare64's factor), floor = (the count c above, the store's 4 and the add's 1
where they apply) U max |reference|: the roundings torch's fp32 path does not have (split residuals at their largest)
or shares, relative to the layer's largest value. A dropped lo product (2^-11 per term, ~2^-11 / sqrt(K) of the
result) is about a hundred times this bar while it hides under the rigorous one's K U sum |w x| only by ~sqrt(K).

Tracked maxima (test_tracked_maxima_cover_the_stored_rows). Rows past M of a partial workgroup repeat row M - 1 in
the forward (mm = min(m, M - 1)) and are exact zeros in the backward, so every tracked maximum is a maximum over stored
rows. Bit equality is required where the kernel reduces the very registers it stores: z_max; act_max[l] of every layer
of the 4-wave ReLU forward (d_hidden 64 / 128 / 256, and 512 under AVR_X3_SAVE_WAVES=4: prep_input / blend_stage take
the max of v, save_layer stores v); grads_max[2 nb] (absmax of dx, store_rows of dx). The 8-wave forward reduces
max_relu_affine in a first pass and recomputes the value it stores in a second: never below, at most one exponent
step above. grads_max[l < 2 nb] is the max of the registers whose (hi + lo) / s_x the row store writes: within
2^-22 of the stored max. Softplus: act_bound(m) = softplus(max(0, max x)) against the stored max softplus(x_i):
equal where max x >= 0 up to the 10 U above (fp32 log1pf(expf(.)) need not be monotone to the last bit), and never
above max(stored max, softplus(0) = ln 2 / beta) by more than that."""
import functools
import types

import numpy as np
import pytest
import torch

import field_train_ref as FR
from oracle import avr_oracle as O
from test_gpu_bn_kernels import POISON, _poisoned, _report, _untouched, _worst
from test_gpu_train import DEV, _net, _points

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, np.float64
U = 2.0 ** -24
TIGHT = 2.0
C_FC, C_STREAM, C_OUT, C_BWD, C_LAST = 13, 23, 22, 8, 3
C_STORE, SP_FWD, SP_BWD = 4, 10, 6
TINY = 2.0 ** -37

D_LATENT, LATENT_HW, N_BLOCKS, COMBINE, N_SCENES = 64, (8, 8), 3, 2, 3
ROWS = [(1, 1), (1, 63), (1, 64), (1, 65), (1, 130), (3, 65)]          # (n_scenes, M per scene)
NETS = [(64, 0.0), (128, 0.0), (256, 0.0), (512, 0.0), (64, 1.5), (512, 1.5)]       # (d_hidden, beta)
# (d_hidden, beta, AVR_X3_SAVE_WAVES, AVR_X3_BWD_WAVES); None: the switch is unset (one layout exists)
LAYOUTS = [(64, 0.0, None, None), (128, 0.0, None, None), (256, 0.0, None, None), (512, 0.0, 8, 8), (512, 0.0, 8, 4),
           (512, 0.0, 4, 8), (512, 0.0, 4, 4), (64, 1.5, None, None), (512, 1.5, None, None)]
MAXIMA_LAYOUTS = [(64, 0.0, None, None), (256, 0.0, None, None), (512, 0.0, 8, 8), (512, 0.0, 4, 4),
                  (64, 1.5, None, None), (512, 1.5, None, None)]
STORE_LAYOUTS = [(64, 0.0, None, None), (512, 0.0, 8, 8), (512, 0.0, 8, 4), (512, 0.0, 4, 4)]
OUTLIER_M = 65
OUTLIER_ROWS = {"first": 0, "middle": OUTLIER_M + 35, "last": N_SCENES * OUTLIER_M - 1}   # of 3 x 65 rows


def _lid(c):
    d, beta, save, bwd = c
    return f"H{d}" + (f"-softplus{beta}" if beta else "") + (f"-save{save}-bwd{bwd}" if save else "")


# ------------------------------------------------------------ inputs (no GPU needed: the CPU test builds them too)
@functools.lru_cache(maxsize=None)
def net_for(d_hidden, beta):
    """Three scenes with their own maps and poses; a launch over n scenes takes the first n."""
    return _net(d_hidden, N_BLOCKS, D_LATENT, LATENT_HW, combine_layer=COMBINE, sb=N_SCENES, beta=beta)


def inputs_for(M):
    """xyz, viewdirs (3, M, 3) and d loss / d out (3, M, 4) of the three scenes, one fixed seed per M."""
    return _points(N_SCENES, M, seed=1000 + M)


def outlier_inputs(row):
    """inputs_for(65) with one outlier row (of the 195): its d loss / d out 2^10 times the rest, its point moved out
    to coordinates of 4 .. 16 in front of the camera, which makes its hidden activations the largest of every layer
    (test_field_train_ref_cpu checks that on the float64 reference)."""
    xyz, vd, go = (t.clone() for t in inputs_for(OUTLIER_M))
    s, m = divmod(row, OUTLIER_M)
    p = xyz[s, m]
    p = torch.sign(p) * (4.0 + 30.0 * p.abs())
    p[2] = p[2].abs()
    xyz[s, m] = p
    go[s, m] *= 2.0 ** 10
    return xyz, vd, go


def weights64(net):
    return {k: v.detach().double().cpu().numpy() for k, v in net.mlp_coarse.state_dict().items() if ".bn_" not in k}


# ------------------------------------------------------------------ launches
def _set_layout(monkeypatch, save, bwd):
    for name, v in (("AVR_X3_SAVE_WAVES", save), ("AVR_X3_BWD_WAVES", bwd)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _bits(x):
    return int(np.float32(x).view(np.int32))


def _floats(words):
    return words.detach().cpu().numpy().view(np.float32).astype(F64)


def _tail_nan(t, rows, width):
    """t's first `rows` rows with two NaN rows directly behind them."""
    buf = torch.full((rows + 2, width), float("nan"), device=DEV, dtype=F32)
    buf[:rows] = t.reshape(-1, width)[:rows].to(DEV)
    return buf


def _launch(net, xyz, vd, go, n_scenes, M, groups=None, guard=False, act_max=None, g_max=None):
    """avr_field_fwd_points_train, then avr_field_bwd, per group of scenes as avr.field._FieldTrain launches them,
    into buffers prefilled with POISON. guard: act_rows = grads_rows = rows + 3, ld_z = padded d_in + 4, 64 guard words
    behind each mask. xyz / viewdirs / grad_out always have NaN rows behind the last scene's row M - 1."""
    import ctypes

    from avr import _lib
    from avr._lib import call, ptr, size_query, stream_of
    fused = net.fused()
    entry = fused.packed(True)
    dims = entry.dims_as(_lib.FIELD_X3)
    bwd = fused.packed_bwd(True, entry)
    tables = fused.tables_batch(True, N_SCENES, fast=True, entry=entry)
    H, nb, d_in = dims.d_hidden, dims.n_blocks, dims.d_in
    n_l, rows = 2 * nb + 1, n_scenes * M
    zs = d_in + (-d_in) % 4
    buf_rows, ld_z, mask_guard = (rows + 3, zs + 4, 64) if guard else (rows, zs, 0)
    R = types.SimpleNamespace(H=H, nb=nb, n_l=n_l, rows=rows, M=M, n_scenes=n_scenes, d_in=d_in, zs=zs, ld_z=ld_z,
                              beta=float(dims.beta), nz=dims.n_lin_z, tables=tables, net=net)
    x_t, v_t = _tail_nan(xyz[:n_scenes], rows, 3), _tail_nan(vd[:n_scenes], rows, 3)
    g_t = _tail_nan(go[:n_scenes], rows, 4)
    R.out, R.act, R.G = _poisoned(rows + 2, 4), _poisoned(n_l, buf_rows, H), _poisoned(n_l, buf_rows, H)
    R.zf = _poisoned(buf_rows, ld_z)
    R.act_max = torch.zeros(n_l + 1, device=DEV, dtype=torch.int32) if act_max is None else act_max   # + z_max
    R.g_max = torch.zeros(n_l, device=DEV, dtype=torch.int32) if g_max is None else g_max
    R.masks, R.grad_out = [], g_t
    stream = stream_of(R.act)
    for g0, n in groups or [(0, n_scenes)]:
        _, mask_n = size_query("avr_field_train_sizes", ctypes.byref(dims), n, M, n=2)
        mask = torch.full((mask_n + mask_guard,), POISON, device=DEV, dtype=torch.int32)
        call("avr_field_fwd_points_train", ctypes.byref(dims), fused.views(range(g0, g0 + n)), n, ptr(entry.packed),
             ptr(tables[g0]), ptr(x_t, g0 * M * 3), ptr(v_t, g0 * M * 3), M, ptr(R.out, g0 * M * 4),
             ptr(R.act, g0 * M * H), buf_rows, ptr(mask), ptr(R.act_max), ptr(R.zf, g0 * M * ld_z), ld_z,
             ptr(R.act_max, n_l), stream)
        R.masks.append((g0, n, mask, mask_n))
    for g0, n, mask, _ in R.masks:
        call("avr_field_bwd", ctypes.byref(dims), ptr(entry.packed), ptr(bwd), n, M, ptr(R.out, g0 * M * 4),
             ptr(g_t, g0 * M * 4), ptr(mask), ptr(R.act, g0 * M * H), buf_rows, ptr(R.G, g0 * M * H), buf_rows,
             ptr(R.g_max), stream)
    torch.cuda.synchronize()
    return R


def _np(t):
    return t.detach().cpu().numpy()


def _blends(R):
    """The float64 bilinear blend of the input lin_z tables' rows (and of their absolute values) at the kernel's own
    xyz_rot: (n_lin_z, rows, H) each."""
    net, M = R.net, R.M
    T = _np(R.tables).astype(F64)                                     # (scenes, tables, h * w, H)
    poses, focal, c = _np(net.poses), _np(net.focal), _np(net.c)      # fp32, what FusedField.view hands the kernel
    scaling, shape = _np(net.encoder.latent_scaling), _np(net.image_shape)
    xr = _np(R.zf)[:R.rows, :3]
    dummy = np.zeros((R.H,) + LATENT_HW, np.float32)                  # (the function takes the map's shape from it)
    bl, ab = np.zeros((R.nz, R.rows, R.H)), np.zeros((R.nz, R.rows, R.H))
    for s in range(R.n_scenes):
        sl = slice(s * M, (s + 1) * M)
        xc = xr[sl] + poses[s][:, 3]                                  # fp32, PixelNeRFField.features' order
        uv = -xc[:, :2] / xc[:, 2:]
        uv = uv * focal[s] + c[s]
        assert uv.dtype == np.float32
        for b in range(R.nz):
            bl[b, sl] = O.grid_sample_bilinear_border(dummy, uv, scaling, shape, rows=T[s, b])
            ab[b, sl] = O.grid_sample_bilinear_border(dummy, uv, scaling, shape, rows=np.abs(T[s, b]))
    return bl, ab


def _tiny(x, Wm):
    """lo halves in fp16's subnormal range: 2^-37 of the tensor's max per element, on either operand.
    x (M, K) rows, Wm (N, K) the weights as the layer applies them (x @ Wm.T)."""
    x, Wm = np.abs(x), np.abs(Wm)
    return TINY * (x.max(initial=0.0) * Wm.sum(1)[None, :] + Wm.max(initial=0.0) * x.sum(1)[:, None])


def _t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _act32(x, beta):
    return torch.nn.functional.softplus(x, beta=beta) if beta > 0 else torch.relu(x)


def _slope32(y, beta):
    return -torch.expm1(-beta * y) if beta > 0 else (y > 0).to(F32)


def _both(worst, name, got, ref, bar, got_t, floor, note_r, note_t):
    """The two bars of one quantity: elementwise err <= bar, and max err <= TIGHT * torch fp32's max err + floor."""
    err = np.abs(got.astype(F64) - ref)
    r = _worst(worst, name + " elementwise", err, bar, note_r)
    eh, et = float(err.max(initial=0.0)), float(np.abs(_np(got_t).astype(F64) - ref).max(initial=0.0))
    t = _worst(worst, name + " layer max", eh, TIGHT * et + floor, note_t)
    return r, t, eh, et


@functools.lru_cache(maxsize=None)
def _weights_of(d_hidden, beta):
    net = net_for(d_hidden, beta)
    W = weights64(net)
    return W, {k: _t32(v) for k, v in W.items()}


# ------------------------------------------------------------------ A. layer by layer, every layout
@pytest.mark.parametrize("n_scenes,M", ROWS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=_lid)
def test_train_forward_layers_vs_float64(layout, n_scenes, M, monkeypatch):
    """avr_field_fwd_points_train's act[l] and out against the local float64 forms, both bars (module docstring)."""
    d_hidden, beta, save, bwd = layout
    _set_layout(monkeypatch, save, bwd)
    net = net_for(d_hidden, beta)
    W, Wt = _weights_of(d_hidden, beta)
    R = _launch(net, *inputs_for(M), n_scenes, M)
    H, nb, rows, sp = R.H, R.nb, R.rows, 1 if beta > 0 else 0
    act_t, zf_t = R.act[:, :rows], R.zf[:rows, :R.d_in]
    act, zf, out = _np(act_t).astype(F64), _np(zf_t).astype(F64), _np(R.out[:rows])
    assert np.isfinite(act).all() and np.isfinite(out).all() and np.isfinite(zf).all()
    bl, ab = _blends(R)
    worst, fails = {}, []

    def check(name, key, *a):
        r, t, eh, et = _both(worst, name, *a)
        if r > 1.0 or t > 1.0:
            fails.append((key, f"elementwise {r:.3f}", f"layer max {t:.3f} (HIP {eh:.2e}, torch fp32 {et:.2e})"))

    # the residual stream: act[2b] = act_fn(x_b), the bar of block b the sum of the steps' bars up to b
    xs, ings = FR.local_stream(zf, bl, ab, act, W, nb)
    cum, cnt, x32, xmax = 0.0, 0, None, 0.0
    for b in range(nb + 1):
        if b == 0:
            K, xop, name = 64, zf, "lin_in"
            x32 = torch.addmm(Wt["lin_in.bias"] + Wt["lin_z.0.bias"], zf_t, Wt["lin_in.weight"].t()) + _t32(bl[0])
        else:
            K, xop, name = H, act[2 * b - 1], f"blocks.{b - 1}.fc_1"
            bias = Wt[name + ".bias"] + (Wt[f"lin_z.{b}.bias"] if b < R.nz else 0.0)
            x32 = x32 + torch.addmm(bias, act_t[2 * b - 1], Wt[name + ".weight"].t())
            if b < R.nz:
                x32 = x32 + _t32(bl[b])
        cum = cum + (K + C_STREAM + sp) * U * ings[b] + _tiny(xop, W[name + ".weight"])
        cnt += C_STREAM + sp
        xmax = max(xmax, float(np.abs(xs[b]).max()))
        ref = FR.act_fn(xs[b], beta)
        check("act[2b] (residual stream)", 2 * b, act[2 * b], ref, cum + sp * SP_FWD * U * np.abs(ref),
              _act32(x32, beta), (cnt * xmax + sp * SP_FWD * float(np.abs(ref).max())) * U,
              "sum over the steps of (K + 23) U (|x_b| + |W| @ |x| + |b| + blend |rows|)",
              "2 x torch fp32 chain + 23 (b + 1) U max |x|")
    for b in range(nb):
        ref, ing = FR.local_fc0(act[2 * b], W, b, beta)
        name = f"blocks.{b}.fc_0"
        bar = (H + C_FC + sp) * U * ing + _tiny(act[2 * b], W[name + ".weight"]) + sp * SP_FWD * U * np.abs(ref)
        got_t = _act32(torch.addmm(Wt[name + ".bias"], act_t[2 * b], Wt[name + ".weight"].t()), beta)
        check("act[2b+1] (fc_0)", 2 * b + 1, act[2 * b + 1], ref, bar, got_t,
              (C_FC + sp + sp * SP_FWD) * U * float(np.abs(ref).max()),
              "(K + 13) U (|W| @ |x| + |b|)", "2 x torch fp32 addmm + 13 U max |ref|")
    ref, ing = FR.local_out(act[2 * nb], W)
    raw_bar = (H + C_OUT) * U * ing + _tiny(act[2 * nb], W["lin_out.weight"])
    bar = raw_bar * np.array([0.25, 0.25, 0.25, 1.0]) + 4 * U * np.array([1.0, 1.0, 1.0, 0.0])
    raw_t = torch.addmm(Wt["lin_out.bias"], act_t[2 * nb], Wt["lin_out.weight"].t())
    got_t = torch.cat([torch.sigmoid(raw_t[:, :3]), torch.relu(raw_t[:, 3:])], -1)
    raw_max = float(np.abs(FR._lin(act[2 * nb], W, "lin_out")).max())
    check("out (lin_out)", "out", out, ref, bar, got_t, (C_OUT * raw_max + 4) * U,
          "(K + 22) U (|W| @ |x| + |b|) (/ 4 + 4 U through the sigmoids)", "2 x torch fp32 + 22 U max |raw| + 4 U")
    _report(f"avr_field_fwd_points_train {_lid(layout)} scenes={n_scenes} M={M}", worst)
    assert not fails, fails


@pytest.mark.parametrize("n_scenes,M", ROWS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=_lid)
def test_backward_layers_vs_float64(layout, n_scenes, M, monkeypatch):
    """avr_field_bwd's G[l] against the local float64 forms of the stored rows, both bars; for ReLU the mask layout
    without a tolerance: a non-zero G[2b] (G[2 nb - 1]) element has a positive act[2b+1] (act[2 nb])."""
    d_hidden, beta, save, bwd = layout
    _set_layout(monkeypatch, save, bwd)
    net = net_for(d_hidden, beta)
    W, Wt = _weights_of(d_hidden, beta)
    R = _launch(net, *inputs_for(M), n_scenes, M)
    H, nb, rows, sp = R.H, R.nb, R.rows, 1 if beta > 0 else 0
    act_t, G_t, out_t, go_t = R.act[:, :rows], R.G[:, :rows], R.out[:rows], R.grad_out[:rows]
    act, G, out, go = (_np(t).astype(F64) for t in (act_t, G_t, out_t, go_t))
    assert np.isfinite(G).all()
    gmax = np.abs(G).reshape(R.n_l, -1).max(1)
    c_b = C_BWD + sp * SP_BWD
    worst, fails = {}, []

    def store(ref, l):      # RowSide's (hi + lo) / s_x of the register value
        return C_STORE * U * np.abs(ref) + TINY * gmax[l]

    def check(name, key, *a):
        r, t, eh, et = _both(worst, name, *a)
        if r > 1.0 or t > 1.0:
            fails.append((key, f"elementwise {r:.3f}", f"layer max {t:.3f} (HIP {eh:.2e}, torch fp32 {et:.2e})"))

    # lin_out^T
    l = 2 * nb - 1
    ref, ing = FR.local_g_last(out, go, act[2 * nb], W, beta)
    d4_t = torch.cat([go_t[:, :3] * ((1.0 - out_t[:, :3]) * out_t[:, :3]), go_t[:, 3:] * (out_t[:, 3:] > 0)], -1)
    got_t = (d4_t @ Wt["lin_out.weight"]) * _slope32(act_t[2 * nb], beta)
    check("G[2nb-1] (lin_out^T)", l, G[l], ref, (4 + C_LAST + sp * SP_BWD) * U * ing + store(ref, l), got_t,
          (C_LAST + sp * SP_BWD + C_STORE) * U * float(np.abs(ref).max()),
          "(4 + 3) U |W_out|^T |d4| + the store's 4 U |ref|", "2 x torch fp32 + 7 U max |ref|")
    if not sp:
        assert not ((G[l] != 0) & ~(act[2 * nb] > 0)).any(), "G[2nb-1] != 0 under a zero act[2nb]: mask layout"
    for b in range(nb - 1, -1, -1):
        # fc_1^T
        ref, ing = FR.local_g_fc0(G[2 * b + 1], act[2 * b + 1], W, b, beta)
        Wm = W[f"blocks.{b}.fc_1.weight"]
        bar = (H + c_b) * U * ing + _tiny(G[2 * b + 1], Wm.T) + store(ref, 2 * b)
        got_t = (G_t[2 * b + 1] @ Wt[f"blocks.{b}.fc_1.weight"]) * _slope32(act_t[2 * b + 1], beta)
        check("G[2b] (fc_1^T)", 2 * b, G[2 * b], ref, bar, got_t, (c_b + C_STORE) * U * float(np.abs(ref).max()),
              "(K + 8) U |G| @ |W1| + the store's 4 U |ref|", "2 x torch fp32 matmul + 12 U max |ref|")
        if not sp:
            assert not ((G[2 * b] != 0) & ~(act[2 * b + 1] > 0)).any(), f"G[{2 * b}] != 0 under a zero act: mask layout"
        # fc_0^T onto the residual gradient
        l = 2 * b - 1 if b > 0 else 2 * nb
        ref, ing = FR.local_g_res(G[2 * b + 1], G[2 * b], act[2 * b], W, b, beta)
        Wm = W[f"blocks.{b}.fc_0.weight"]
        bar = ((H + c_b) * U * ing + _tiny(G[2 * b], Wm.T) + store(G[2 * b + 1], 2 * b + 1) + U * np.abs(ref)
               + (store(ref, l) if b > 0 else 0.0))
        got_t = G_t[2 * b + 1] + (G_t[2 * b] @ Wt[f"blocks.{b}.fc_0.weight"]) * _slope32(act_t[2 * b], beta)
        cnt = c_b + C_STORE + 1 + (C_STORE if b > 0 else 0)
        check("G[2b-1], G[2nb] (fc_0^T + residual)", l, G[l], ref, bar, got_t, cnt * U * float(np.abs(ref).max()),
              "(K + 8) U |G| @ |W0| + 4 U |G[2b+1]| + U |ref| + the store's 4 U |ref|",
              "2 x torch fp32 + 17 U max |ref|")
    _report(f"avr_field_bwd {_lid(layout)} scenes={n_scenes} M={M}", worst)
    assert not fails, fails


# ------------------------------------------------------------------ B. the tracked maxima
def _exp_steps(tracked, stored):
    return int(np.frexp(tracked)[1] - np.frexp(stored)[1])


def _check_maxima(R, save, prefix):
    """act_max / z_max / grads_max of a launch from zeroed words against the rows it stored."""
    rows, nb, n_l = R.rows, R.nb, R.n_l
    act = np.abs(_np(R.act[:, :rows])).reshape(n_l, -1).max(1)
    G = np.abs(_np(R.G[:, :rows])).reshape(n_l, -1).max(1)
    zf = np.abs(_np(R.zf[:rows, :R.d_in])).max()
    am_w, gm_w = _np(R.act_max), _np(R.g_max)
    am, gm = _floats(R.act_max), _floats(R.g_max)
    assert np.isfinite(am).all() and np.isfinite(gm).all(), (prefix, am, gm)
    assert int(am_w[n_l]) == _bits(zf), (prefix, "z_max is the max of the stored z_feature rows", am[n_l], zf)
    for l in range(n_l):
        if R.beta > 0:
            slack = 1 + SP_FWD * U
            assert am[l] * slack >= act[l], (prefix, "act_max below the stored rows", l, am[l], act[l])
            assert am[l] <= max(act[l], np.log(2.0) / R.beta) * slack, (prefix, "act_bound's slack", l, am[l], act[l])
        elif save == 8:
            assert am[l] >= act[l], (prefix, "act_max below the stored rows", l, am[l], act[l])
        else:
            assert int(am_w[l]) == _bits(act[l]), (prefix, "act_max is the max of the stored rows", l, am[l], act[l])
        assert 0 <= _exp_steps(am[l], act[l]) <= 1, (prefix, "act_max costs more than one exponent step", l)
        if l == 2 * nb:
            assert int(gm_w[l]) == _bits(G[l]), (prefix, "grads_max[2nb] is the max of the stored rows", gm[l], G[l])
        else:
            assert gm[l] * (1 + 2.0 ** -22) >= G[l], (prefix, "grads_max below the stored rows", l, gm[l], G[l])
            assert gm[l] <= G[l] * (1 + 2.0 ** -22), (prefix, "grads_max above the stored rows", l, gm[l], G[l])
        assert -1 <= _exp_steps(gm[l], G[l]) <= 1, (prefix, "grads_max costs more than one exponent step", l)


@pytest.mark.parametrize("where", list(OUTLIER_ROWS))
@pytest.mark.parametrize("layout", MAXIMA_LAYOUTS, ids=_lid)
def test_tracked_maxima_cover_the_stored_rows(layout, where, monkeypatch):
    """One outlier row (row 0; a middle scene; the last row, alone in its workgroup) among 3 x 65: the tracked maxima
    against the stored rows (module docstring), the prefill and accumulation semantics of the words, and
    avr_weight_grads on the TRACKED words against a float64 G^T act of the stored rows."""
    from avr import ops
    d_hidden, beta, save, bwd = layout
    _set_layout(monkeypatch, save, bwd)
    net = net_for(d_hidden, beta)
    xyz, vd, go = outlier_inputs(OUTLIER_ROWS[where])
    M = OUTLIER_M
    R = _launch(net, xyz, vd, go, N_SCENES, M)
    rows, nb, n_l = R.rows, R.nb, R.n_l
    _check_maxima(R, save, "one launch")
    # the outlier is what the maxima come from
    row = OUTLIER_ROWS[where]
    for name, t in (("act", R.act), ("G", R.G)):
        per_row = _np(t[:, :rows]).astype(F64)
        per_row = np.abs(per_row).max(2)
        assert (per_row.argmax(1) == row).all(), (name, "the outlier row does not hold every max", per_row.argmax(1))
    # prefill: a larger word stays (even l), a smaller one is replaced by the launch's own max (odd l, z_max)
    am, gm = _floats(R.act_max), _floats(R.g_max)
    am_p = torch.tensor([_bits(2 * am[l]) if l % 2 == 0 and l < n_l else _bits(0.5 * am[l]) for l in range(n_l + 1)],
                        device=DEV, dtype=torch.int32)
    gm_p = torch.tensor([_bits(2 * gm[l]) if l % 2 == 0 else _bits(0.5 * gm[l]) for l in range(n_l)],
                        device=DEV, dtype=torch.int32)
    want_a, want_g = _np(am_p).copy(), _np(gm_p).copy()
    want_a[1::2], want_g[1::2] = _np(R.act_max)[1::2], _np(R.g_max)[1::2]
    P = _launch(net, xyz, vd, go, N_SCENES, M, act_max=am_p, g_max=gm_p)
    assert np.array_equal(_np(P.act_max), want_a), ("act_max prefill", _floats(P.act_max), am)
    assert np.array_equal(_np(P.g_max), want_g), ("grads_max prefill", _floats(P.g_max), gm)
    # two group launches into one set of words accumulate (avr.field._FieldTrain over scene_groups)
    S = _launch(net, xyz, vd, go, N_SCENES, M, groups=[(0, 2), (2, 1)])
    assert torch.equal(S.act_max, R.act_max) and torch.equal(S.g_max, R.g_max), "two launches: other maxima"
    assert torch.equal(S.act[:, :rows], R.act[:, :rows]) and torch.equal(S.G[:, :rows], R.G[:, :rows])
    _check_maxima(S, save, "two launches")
    # avr_weight_grads of the fc layers on the tracked words
    lay = [(R.G[k, :rows], R.act[k, :rows], R.g_max[k:k + 1], R.act_max[k:k + 1], True) for k in range(2 * nb)]
    res = ops.weight_grads(lay, rows)
    torch.cuda.synchronize()
    worst = {}
    for k, (dW, db) in enumerate(res):
        dW_r, db_r = FR.weight_grads(_np(R.G[k, :rows]), _np(R.act[k, :rows]))
        for name, got, ref in (("dW", _np(dW), dW_r), ("db", _np(db), db_r)):
            assert np.isfinite(got).all(), (k, name, "not finite: the split scale overflowed")
            e = _worst(worst, name, float(np.abs(got - ref).max()), 2e-6 * float(np.abs(ref).max()),
                       "2e-6 max |G^T act| (test_weight_grads_kernel_vs_fp64's bar)")
            assert e <= 1.0, (k, name, e)
    _report(f"avr_weight_grads on tracked maxima {_lid(layout)} outlier {where}", worst)


# ------------------------------------------------------------------ C. bounds of every store
@pytest.mark.parametrize("n_scenes,M", ROWS)
@pytest.mark.parametrize("layout", STORE_LAYOUTS, ids=_lid)
def test_training_stores_stay_inside_their_rows(layout, n_scenes, M, monkeypatch):
    """act_rows = grads_rows = rows + 3, ld_z = padded d_in + 4, guard words behind mask_words, NaN rows behind the
    last input row: every guard is untouched, the z_feature padding is zero, everything stored is finite."""
    d_hidden, beta, save, bwd = layout
    _set_layout(monkeypatch, save, bwd)
    net = net_for(d_hidden, beta)
    R = _launch(net, *inputs_for(M), n_scenes, M, guard=True)
    rows = R.rows
    assert R.act.shape[1] == rows + 3 and R.ld_z == R.zs + 4
    for l in range(R.n_l):
        assert _untouched(R.act[l, rows:]), f"act[{l}]: rows past the last were written"
        assert _untouched(R.G[l, rows:]), f"G[{l}]: rows past the last were written"
        assert not (R.act[l, :rows].view(torch.int32) == POISON).any(), f"act[{l}]: a row was not written"
        assert not (R.G[l, :rows].view(torch.int32) == POISON).any(), f"G[{l}]: a row was not written"
    assert _untouched(R.zf[rows:]) and _untouched(R.out[rows:]), "z_feature / out: rows past the last were written"
    for _, _, mask, mask_n in R.masks:
        assert bool((mask[mask_n:] == POISON).all()), "words behind mask_words were written"
    zf = _np(R.zf[:rows])
    assert not zf[:, R.d_in:].any(), "z_feature columns d_in .. ld_z - 1 are not zero"
    for name, t in (("out", R.out[:rows]), ("act", R.act[:, :rows]), ("G", R.G[:, :rows]), ("z_feature", R.zf[:rows])):
        assert bool(torch.isfinite(t).all()), name
    assert np.isfinite(_floats(R.act_max)).all() and np.isfinite(_floats(R.g_max)).all()
    # the padded layout changes no value
    Q = _launch(net, *inputs_for(M), n_scenes, M)
    assert torch.equal(Q.act, R.act[:, :rows]) and torch.equal(Q.G, R.G[:, :rows])
    assert torch.equal(Q.out[:rows], R.out[:rows]) and torch.equal(Q.zf[:, :R.d_in], R.zf[:rows, :R.d_in])
    assert torch.equal(Q.act_max, R.act_max) and torch.equal(Q.g_max, R.g_max)
