"""Reference of the training-mode BatchNorm path's kernels (csrc/bn_train.hip: avr_bn_layer_run, avr_bn_stats,
avr_bn_grad_stats, avr_bn_grad_rows) in plain numpy, float64 (np.longdouble where sums could cancel). Nothing here
imports avr or torch: the contract of include/avr.h ("training-mode BatchNorm") is restated, not the kernels' order
of operations.

Rows are split into workgroups of 64 (ROWS); the last one has M - 64 (nwg - 1) rows. A forward partial is a
workgroup's per-column (mean, M2 = sum of squared deviations about that mean); a backward partial is its per-column
(sum gp, sum gp * xhat), xhat = (pre - mu) * invstd.

The forward statistics are combined in a form that cannot cancel (a pivot c, then deviations only):

    mean = c + sum_i n_i (p0_i - c) / M,  c = p0_0        M2 = sum_i p1_i + sum_i n_i (p0_i - mean)^2

which is deliberately not the kernel's sum (p1 + n p0^2) - M mean^2. invstd uses the biased variance M2 / M (the
normalisation), the running variance the unbiased M2 / (M - 1), as torch's batch_norm does.

Weights are the raw nn.Linear matrices W (out_dim, in_dim), not a packed blob: forward out = op . W^T + bias,
backward gp = op . W."""
import numpy as np

ROWS = 64
LD = np.longdouble
F64 = np.float64


def n_groups(M):
    return (int(M) + ROWS - 1) // ROWS


def group_sizes(M):
    """Rows of each 64-row workgroup of M rows: 64, ..., 64, M - 64 (nwg - 1)."""
    nwg = n_groups(M)
    n = np.full(nwg, ROWS, dtype=np.int64)
    n[-1] = int(M) - ROWS * (nwg - 1)
    return n


def _vec(v, dtype=F64):
    return None if v is None else np.asarray(v, dtype=dtype)


def combine(p0, p1, M):
    """The batch (mean, M2) of M rows from the (nwg, C) per-workgroup (mean, M2), np.longdouble, cancellation-free."""
    p0, p1 = np.asarray(p0, dtype=LD), np.asarray(p1, dtype=LD)
    n = group_sizes(M).astype(LD)[:, None]
    assert p0.shape == p1.shape and p0.shape[0] == n.shape[0], (p0.shape, p1.shape, M)
    c = p0[0]
    mean = c + (n * (p0 - c)).sum(0) / LD(int(M))
    return mean, p1.sum(0) + (n * (p0 - mean) ** 2).sum(0)


def stats_from_partials(p0, p1, M, gamma, eps, momentum, running_mean=None, running_var=None):
    """avr_bn_stats: the (nwg, C) forward partials p0 (means), p1 (M2) of M rows -> (mu, invstd, scale,
    running_mean', running_var') in float64 (the running pair None where none was passed)."""
    mean, M2 = combine(p0, p1, M)
    Ml = LD(int(M))
    var = M2 / Ml
    invstd = 1.0 / np.sqrt(var + LD(eps))
    scale = np.asarray(gamma, dtype=LD) * invstd
    rm = rv = None
    if running_mean is not None:
        unb = M2 / (Ml - 1) if M > 1 else var
        mom = LD(momentum)
        rm = mom * mean + (1 - mom) * np.asarray(running_mean, dtype=LD)
        rv = mom * unb + (1 - mom) * np.asarray(running_var, dtype=LD)
    return tuple(None if v is None else v.astype(F64) for v in (mean, invstd, scale, rm, rv))


def grad_stats_from_partials(p0, p1, M, gamma, invstd, dgamma0, dbeta0):
    """avr_bn_grad_stats: the (nwg, C) backward partials p0 (sum gp), p1 (sum gp * xhat) ->
    (coef = gamma * invstd, m1 = sum p0 / M, m2 = sum p1 / M, dgamma0 + sum p1, dbeta0 + sum p0) in float64."""
    s0 = np.asarray(p0, dtype=LD).sum(0)
    s1 = np.asarray(p1, dtype=LD).sum(0)
    Ml = LD(int(M))
    coef = _vec(gamma) * _vec(invstd)
    return (coef, (s0 / Ml).astype(F64), (s1 / Ml).astype(F64),
            (np.asarray(dgamma0, dtype=LD) + s1).astype(F64), (np.asarray(dbeta0, dtype=LD) + s0).astype(F64))


def grad_rows(g, pre, res, coef, m1, m2, mu, invstd):
    """avr_bn_grad_rows and the AVR_BN_GRAD operand: res + coef * (g - m1 - (pre - mu) * invstd * m2), res may be
    None. (rows, C) float64."""
    xhat = (_vec(pre) - _vec(mu)) * _vec(invstd)
    out = _vec(coef) * (_vec(g) - _vec(m1) - xhat * _vec(m2))
    return out if res is None else _vec(res) + out


def bn_pre_relu(x, mu, scale, shift):
    """(x - mu) * scale + shift: the value whose sign is the relu mask of AVR_BN_RELU / AVR_BN_BWD."""
    return (_vec(x) - _vec(mu)) * _vec(scale) + _vec(shift)


def relu_operand(src, mu, scale, shift):
    """The AVR_BN_RELU operand relu((src - mu) * scale + shift)."""
    return np.maximum(bn_pre_relu(src, mu, scale, shift), 0.0)


def group_stats(rows):
    """Per 64-row workgroup (mean, M2 about it) of the columns of rows (M, C) -> two (nwg, C) float64 arrays; the
    last workgroup's over its own rows only."""
    rows = np.asarray(rows, dtype=LD)
    M = rows.shape[0]
    mean = np.empty((n_groups(M), rows.shape[1]), dtype=LD)
    M2 = np.empty_like(mean)
    for w in range(mean.shape[0]):
        r = rows[ROWS * w:ROWS * (w + 1)]
        mean[w] = r.sum(0) / LD(r.shape[0])
        M2[w] = ((r - mean[w]) ** 2).sum(0)
    return mean.astype(F64), M2.astype(F64)


def group_grad_sums(gp, pre, mu, invstd):
    """Per 64-row workgroup (sum gp, sum gp * xhat), xhat = (pre - mu) * invstd -> two (nwg, C) float64 arrays."""
    gp = np.asarray(gp, dtype=LD)
    xhat = (np.asarray(pre, dtype=LD) - np.asarray(mu, dtype=LD)) * np.asarray(invstd, dtype=LD)
    nwg = n_groups(gp.shape[0])
    s1 = np.empty((nwg, gp.shape[1]), dtype=LD)
    s2 = np.empty_like(s1)
    for w in range(nwg):
        sl = slice(ROWS * w, ROWS * (w + 1))
        s1[w] = gp[sl].sum(0)
        s2[w] = (gp[sl] * xhat[sl]).sum(0)
    return s1.astype(F64), s2.astype(F64)


def layer_fwd(src, W, bias, in_stats=None, add1=None, operand=None):
    """avr_bn_layer, AVR_BN_FWD: out = W . op + bias (+ add1), op = src (in_stats None: AVR_BN_PLAIN) or
    relu((src - mu) * scale + shift) (in_stats = (mu, scale, shift): AVR_BN_RELU), or `operand` where one is given
    (the operand as a kernel stored it). -> (op, out, (mean, M2) per workgroup of out)."""
    if operand is not None:
        op = _vec(operand)
    elif in_stats is None:
        op = _vec(src)
    else:
        op = relu_operand(src, *in_stats)
    out = op @ _vec(W).T
    if bias is not None:
        out = out + _vec(bias)
    if add1 is not None:
        out = out + _vec(add1)
    return op, out, group_stats(out)


def layer_bwd(src, W, pre_rows, out_stats, grad_in=None, add1=None, operand=None):
    """avr_bn_layer, AVR_BN_BWD: gp = (W^T . op) * [(pre_rows - out_mu) * out_scale + out_shift > 0], out = gp
    (+ add1), with out_stats = (out_mu, out_invstd, out_scale, out_shift). op = src (grad_in None: AVR_BN_PLAIN) or
    the BatchNorm backward of src (grad_in = (src_pre, src_res or None, in_mu, in_invstd, in_scale, in_m1, in_m2):
    AVR_BN_GRAD, in_scale being coef), or `operand`. -> (op, gp, out, (sum gp, sum gp * xhat) per workgroup)."""
    if operand is not None:
        op = _vec(operand)
    elif grad_in is None:
        op = _vec(src)
    else:
        src_pre, src_res, in_mu, in_invstd, in_scale, in_m1, in_m2 = grad_in
        op = grad_rows(src, src_pre, src_res, in_scale, in_m1, in_m2, in_mu, in_invstd)
    out_mu, out_invstd, out_scale, out_shift = out_stats
    mask = bn_pre_relu(pre_rows, out_mu, out_scale, out_shift) > 0
    gp = (op @ _vec(W)) * mask
    out = gp if add1 is None else gp + _vec(add1)
    return op, gp, out, group_grad_sums(gp, pre_rows, out_mu, out_invstd)
