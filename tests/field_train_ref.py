"""float64 restatement (numpy) of the fused field-training path's layer algebra: the ResnetFC of
csrc/field_bwd.hip's header comment and include/avr.h's "field training" block -- avr_field_fwd_points_train's saved
rows act[l] and its output, avr_field_bwd's G[l] -- for a net given as a dict W of float64 arrays under the module's
parameter names (lin_in, blocks.b.fc_0 / fc_1, lin_z.b, lin_out; .weight (out, in) and .bias).

Two parts:
  - the plain chain, forward() / backward(), held to torch float64 autograd by tests/test_field_train_ref_cpu.py;
  - the *local* forms tests/test_gpu_field_train_kernels.py compares the kernels with. Each takes the rows the kernel
    itself stored as its operands, so a comparison spans one GEMM and no error compounds through the weights. Each
    returns (reference, ingredient): ingredient = |W| @ |x| + |b| elementwise, what a rounding-count bar multiplies.

Layer numbering (2 nb + 1 layers): act[2b] = act_fn(x_b) into fc_0 of block b, act[2b+1] = act_fn(fc_0 out) into fc_1,
act[2 nb] = act_fn(x_nb) into lin_out; G[2b] = d loss / d fc_0[b] output, G[2b+1] = d loss / d fc_1[b] output (the
gradient at block b's output), G[2 nb] = d loss / d lin_in output (the gradient at block 0's input).
Geometry (rotation, positional encoding, uv, corner weights) is not restated here: the callers take it from `oracle`."""
import numpy as np

F64 = np.float64


def _a(x):
    return np.asarray(x, F64)


def act_fn(x, beta=0.0):
    """ReLU (beta 0), or Softplus(beta) as torch evaluates it: x where beta x > 20, else log1p(exp(beta x)) / beta."""
    x = _a(x)
    if not beta > 0:
        return np.maximum(x, 0.0)
    bx = x * beta
    return np.where(bx > 20.0, x, np.log1p(np.exp(np.minimum(bx, 20.0))) / beta)


def act_slope(pre, beta=0.0):
    """d act_fn / d x at the pre-activation: [x > 0], or torch's softplus_backward factor (1 where beta x > 20)."""
    pre = _a(pre)
    if not beta > 0:
        return (pre > 0).astype(F64)
    bx = pre * beta
    z = np.exp(np.minimum(bx, 20.0))
    return np.where(bx > 20.0, 1.0, z / (z + 1.0))


def slope_of_act(y, beta=0.0):
    """The same slope from the activation's VALUE y = act_fn(x), as the backward kernel takes it from the saved rows:
    [y > 0] for ReLU, sigmoid(beta x) = 1 - exp(-beta y) for Softplus (no threshold: 1 - e^-20 where torch says 1)."""
    y = _a(y)
    if not beta > 0:
        return (y > 0).astype(F64)
    return -np.expm1(-beta * y)


def n_lin_z(W):
    n = 0
    while f"lin_z.{n}.weight" in W:
        n += 1
    return n


def _lin(x, W, name):
    return _a(x) @ _a(W[name + ".weight"]).T + _a(W[name + ".bias"])


def out_act(raw):
    """(sigmoid, sigmoid, sigmoid, relu) of lin_out's four outputs."""
    raw = _a(raw)
    return np.concatenate([1.0 / (1.0 + np.exp(-raw[:, :3])), np.maximum(raw[:, 3:4], 0.0)], -1)


def d_out(out, grad_out):
    """d loss / d lin_out's raw outputs from the saved out: g (1 - y) y for the sigmoids, g [y > 0] for the relu."""
    out, g = _a(out), _a(grad_out)
    return np.concatenate([g[:, :3] * ((1.0 - out[:, :3]) * out[:, :3]), g[:, 3:4] * (out[:, 3:4] > 0)], -1)


# ------------------------------------------------------------------ the plain chain
def forward(z_feature, lat_blend, W, n_blocks, beta=0.0):
    """z_feature (M, d_in) and lat_blend (M, d_latent), the interpolated latent rows lin_z[b] applies to ->
    dict(x=[x_0 .. x_nb] the residual stream at every block's input and after the last block, pre=[2 nb + 1] the
    pre-activation of every act layer, act=[2 nb + 1], raw (M, 4), out (M, 4))."""
    nz = n_lin_z(W)
    x = _lin(z_feature, W, "lin_in")
    xs, pre = [], []
    for b in range(n_blocks):
        if b < nz:
            x = x + _lin(lat_blend, W, f"lin_z.{b}")
        xs.append(x)
        net = _lin(act_fn(x, beta), W, f"blocks.{b}.fc_0")
        pre += [x, net]
        x = x + _lin(act_fn(net, beta), W, f"blocks.{b}.fc_1")
    xs.append(x)
    pre.append(x)
    act = [act_fn(p, beta) for p in pre]
    raw = _lin(act[-1], W, "lin_out")
    return dict(x=xs, pre=pre, act=act, raw=raw, out=out_act(raw))


def backward(fwd, grad_out, W, n_blocks, beta=0.0):
    """G[0 .. 2 nb] of forward()'s result for d loss / d out = grad_out (M, 4)."""
    pre = fwd["pre"]
    G = [None] * (2 * n_blocks + 1)
    dx = (d_out(fwd["out"], grad_out) @ _a(W["lin_out.weight"])) * act_slope(pre[2 * n_blocks], beta)
    for b in range(n_blocks - 1, -1, -1):
        G[2 * b + 1] = dx
        G[2 * b] = (dx @ _a(W[f"blocks.{b}.fc_1.weight"])) * act_slope(pre[2 * b + 1], beta)
        dx = dx + (G[2 * b] @ _a(W[f"blocks.{b}.fc_0.weight"])) * act_slope(pre[2 * b], beta)
    G[2 * n_blocks] = dx
    return G


def weight_grads(G, X):
    """dW = G^T X (out, in) and db = column sums of G, of one linear layer over the rows."""
    G, X = _a(G), _a(X)
    return G.T @ X, G.sum(0)


# ------------------------------------------------------------------ the local forms
def _abs_lin(x, W, name):
    return np.abs(_a(x)) @ np.abs(_a(W[name + ".weight"])).T + np.abs(_a(W[name + ".bias"]))


def local_fc0(act_in, W, b, beta=0.0):
    """act[2b+1] = act_fn(W0_b . act[2b] + b0_b) from the stored act[2b] rows."""
    name = f"blocks.{b}.fc_0"
    return act_fn(_lin(act_in, W, name), beta), _abs_lin(act_in, W, name)


def local_stream(z_feature, blends, abs_blends, act, W, n_blocks):
    """The residual stream from the stored rows: x_0 = lin_in(z_feature) + lin_z[0].bias + blends[0],
    x_{b+1} = x_b + W1_b . act[2b+1] + b1_b + lin_z[b+1].bias + blends[b+1] (blends[b] (M, d_hidden) = the bilinear
    blend of lin_z[b]'s bias-free table rows, abs_blends[b] = the same blend of their absolute values; both lists are
    n_lin_z long). -> ([x_0 .. x_nb], [ingredient of each step]): the ingredient of step b + 1 includes |x_b|, the
    accumulator the GEMM adds onto. act[2b+2] is compared with act_fn(x_{b+1}); its bar is the sum of the steps' bars
    up to b + 1 (the activations are 1-Lipschitz)."""
    nz = len(blends)
    x = _lin(z_feature, W, "lin_in")
    ing = _abs_lin(z_feature, W, "lin_in")
    if nz > 0:
        x = x + _a(W["lin_z.0.bias"]) + _a(blends[0])
        ing = ing + np.abs(_a(W["lin_z.0.bias"])) + _a(abs_blends[0])
    xs, ings = [x], [ing]
    for b in range(n_blocks):
        name = f"blocks.{b}.fc_1"
        ing = np.abs(x) + _abs_lin(act[2 * b + 1], W, name)
        x = x + _lin(act[2 * b + 1], W, name)
        if b + 1 < nz:
            x = x + _a(W[f"lin_z.{b + 1}.bias"]) + _a(blends[b + 1])
            ing = ing + np.abs(_a(W[f"lin_z.{b + 1}.bias"])) + _a(abs_blends[b + 1])
        xs.append(x)
        ings.append(ing)
    return xs, ings


def local_out(act_last, W):
    """out = (sigmoid, sigmoid, sigmoid, relu)(W_out . act[2 nb] + b_out). -> (out, ingredient of the raw outputs)."""
    return out_act(_lin(act_last, W, "lin_out")), _abs_lin(act_last, W, "lin_out")


def local_g_last(out, grad_out, act_last, W, beta=0.0):
    """G[2 nb - 1] = (W_out^T d4) (.) act'(act[2 nb]), d4 from the stored out."""
    d4, Wo = d_out(out, grad_out), _a(W["lin_out.weight"])
    s = slope_of_act(act_last, beta)
    return (d4 @ Wo) * s, (np.abs(d4) @ np.abs(Wo)) * s


def local_g_fc0(g1, act1, W, b, beta=0.0):
    """G[2b] = (W1_b^T G[2b+1]) (.) act'(act[2b+1]) from the stored G[2b+1] and act[2b+1] rows."""
    W1 = _a(W[f"blocks.{b}.fc_1.weight"])
    s = slope_of_act(act1, beta)
    return (_a(g1) @ W1) * s, (np.abs(_a(g1)) @ np.abs(W1)) * s


def local_g_res(g1, g0, act0, W, b, beta=0.0):
    """The gradient at block b's input, G[2b-1] (b >= 1) or G[2 nb] (b = 0):
    G[2b+1] + (W0_b^T G[2b]) (.) act'(act[2b]) from the stored rows. -> (reference, GEMM ingredient alone)."""
    W0 = _a(W[f"blocks.{b}.fc_0.weight"])
    s = slope_of_act(act0, beta)
    return _a(g1) + (_a(g0) @ W0) * s, (np.abs(_a(g0)) @ np.abs(W0)) * s
