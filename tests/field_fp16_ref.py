"""CPU reference for the field's "fp16" inference precision (numpy, float64).

RefField wraps an oracle.avr_oracle.PixelNeRFField: it takes the MLP's inputs from that field's features() (the
interpolated latent and z_feature, fp32 as the oracle computes them) and runs the ResnetFC in float64 in one of two
modes:

  "f64"  every operand exact: the oracle's own function with float64 arithmetic;
  "e16"  the inputs and the weights of the rounded layers -- lin_in, fc_0 and fc_1 of every block, lin_out: the
         layers the AVR_FIELD_FP16 kernels round (include/avr.h) -- rounded to fp16, to nearest even, under a
         power-of-two scale that maps the tensor's max |value| into [2^13, 2^14) (pow2_scale_for of the kernels);
         products and sums in float64; biases, the lin_z projections and the residual stream exact.

One scale per tensor: the kernels take one s_w per layer and one s_x per layer and 64-sample workgroup. A power-of-two
scale commutes with rounding to nearest outside the subnormal range (x * 2^k has the significand of x), so the
grouping does not matter as long as no scaled value falls below 2^-14: grouping the rows in blocks of 64 or taking
all of them at once gave bit-identical results on the goldens' 384 points (checked when this file was written, and
again by test_field_fp16_ref_cpu.test_scale_grouping_is_immaterial).
"""
import numpy as np

F64 = np.float64


def round_fp16(x):
    """x (float64) -> fp16(x * s) / s, round to nearest even, s = 2^k with max |x| * s in [2^13, 2^14)."""
    x = np.asarray(x, F64)
    m = float(np.abs(x).max()) if x.size else 0.0
    if not (m > 0.0) or not np.isfinite(m):
        return x
    s = 2.0 ** (14 - np.frexp(m)[1])
    return (x * s).astype(np.float16).astype(F64) / s   # numpy converts float64 -> float16 to nearest even


def _linear(x, W, b, rounded, rows_per_scale=None):
    x, W = np.asarray(x, F64), np.asarray(W, F64)
    if rounded:
        W = round_fp16(W)
        if rows_per_scale:
            x = np.concatenate([round_fp16(x[i:i + rows_per_scale]) for i in range(0, len(x), rows_per_scale)], 0)
        else:
            x = round_fp16(x)
    return x @ W.T + np.asarray(b, F64)


def resnetfc(lat, zf, p, n_blocks, combine_layer, mode, rows_per_scale=None):
    """ResnetFC.forward for ReLU nets without BatchNorm / use_spade, one source view: (B, 4) pre-activation."""
    assert mode in ("f64", "e16")
    r = mode == "e16"
    relu = lambda v: np.maximum(v, 0.0)   # noqa: E731
    lin = lambda v, name: _linear(v, p[name + ".weight"], p[name + ".bias"], r, rows_per_scale)   # noqa: E731
    x = lin(zf, "lin_in")
    for b in range(n_blocks):
        if lat.shape[1] > 0 and b < combine_layer:
            x = x + _linear(lat, p[f"lin_z.{b}.weight"], p[f"lin_z.{b}.bias"], False)
        net = lin(relu(x), f"blocks.{b}.fc_0")
        x = x + lin(relu(net), f"blocks.{b}.fc_1")
    return lin(relu(x), "lin_out")


class RefField:
    """field(xyz, viewdirs, coarse) -> (..., 4) float64 (sigmoid rgb, relu sigma), the call protocol of the oracle's
    fields (oracle.avr_oracle.render takes it)."""

    def __init__(self, oracle_field, mode, rows_per_scale=None):
        assert oracle_field.beta == 0.0
        self.f, self.mode, self.rows_per_scale = oracle_field, mode, rows_per_scale

    def __call__(self, xyz, viewdirs, coarse=True):
        shp = np.asarray(xyz).shape
        lat, zf = self.f.features(xyz, viewdirs)
        p = self.f.pc if coarse else self.f.pf
        out = resnetfc(np.asarray(lat, F64), np.asarray(zf, F64), p, self.f.n_blocks, self.f.combine_layer, self.mode,
                       self.rows_per_scale)
        res = np.concatenate([1.0 / (1.0 + np.exp(-out[:, :3])), np.maximum(out[:, 3:4], 0.0)], -1)
        return res.reshape(shp[:-1] + (4,))


def errors(out, gold):
    """(rgb mean, rgb max, sigma mean, sigma max) absolute error of out against gold, both (..., 4)."""
    d = np.abs(np.asarray(out, F64) - np.asarray(gold, F64)).reshape(-1, 4)
    return float(d[:, :3].mean()), float(d[:, :3].max()), float(d[:, 3].mean()), float(d[:, 3].max())
