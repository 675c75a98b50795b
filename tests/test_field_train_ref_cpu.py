"""tests/field_train_ref.py (the float64 reference the fused field-training kernels are held to) against torch float64
autograd of the module path (net.double(), use_fused = False), for every net tests/test_gpu_field_train_kernels.py
uses, at 3 scenes x 65 rows: every hidden activation (forward pre-hooks on the linear layers), the output, the
gradient at every layer output (tensor hooks) and the fc layers' weight gradients within 1e-12 of each array's max.

And, on the reference alone, what the GPU file's fixed seeds must give for its exact checks to mean something:
no ReLU pre-activation in (0, 2^-30 of its layer's max] (a stored activation could be 0 under a set mask bit once
the fp16 hi half flushes), zeros and positives in every ReLU layer of every 64-row workgroup (a mask word of all ones
or all zeros cannot pass), and the outlier row of the maxima test holding the max of every act and G layer."""
import numpy as np
import pytest
import torch

import field_train_ref as FR
from test_gpu_field_train_kernels import (MAXIMA_LAYOUTS, N_BLOCKS, N_SCENES, NETS, OUTLIER_M, OUTLIER_ROWS, ROWS,
                                          inputs_for, net_for, outlier_inputs, weights64)
from test_gpu_train import _fp64

BAR = 1e-12


def _reference(net, beta, xyz, vd, go):
    """field_train_ref's plain chain on the module's own float64 MLP inputs: (forward dict, G list, W)."""
    def inputs():
        with torch.no_grad():
            lat, zf = net.mlp_inputs(xyz.double(), vd.double())
        return lat.numpy(), zf.numpy(), weights64(net)
    lat, zf, W = _fp64(net, inputs)
    fwd = FR.forward(zf, lat, W, N_BLOCKS, beta)
    return fwd, FR.backward(fwd, go.double().reshape(-1, 4).numpy(), W, N_BLOCKS, beta), W


def _torch_layers(net, xyz, vd, go):
    """The module path in float64 with hooks: act[l] (the linear layers' inputs), out, G[l] (the gradient at the
    linear layers' outputs), and the parameter gradients."""
    mlp, nb = net.mlp_coarse, N_BLOCKS
    act, G, handles = {}, {}, []

    def keep_input(l):
        return lambda mod, args: act.__setitem__(l, args[0].detach().reshape(-1, args[0].shape[-1]).numpy().copy())

    def keep_grad(l):
        def hook(mod, args, output):
            output.register_hook(lambda g: G.__setitem__(l, g.detach().reshape(-1, g.shape[-1]).numpy().copy()))
        return hook

    def run():
        for b, blk in enumerate(mlp.blocks):
            handles.extend([blk.fc_0.register_forward_pre_hook(keep_input(2 * b)),
                            blk.fc_1.register_forward_pre_hook(keep_input(2 * b + 1)),
                            blk.fc_0.register_forward_hook(keep_grad(2 * b)),
                            blk.fc_1.register_forward_hook(keep_grad(2 * b + 1))])
        handles.extend([mlp.lin_out.register_forward_pre_hook(keep_input(2 * nb)),
                        mlp.lin_in.register_forward_hook(keep_grad(2 * nb))])
        try:
            net.zero_grad(set_to_none=True)
            out = net(xyz.double(), coarse=True, viewdirs=vd.double())
            (out * go.double()).sum().backward()
        finally:
            for h in handles:
                h.remove()
        grads = {k: p.grad.detach().numpy().copy() for k, p in mlp.named_parameters() if p.grad is not None}
        net.zero_grad(set_to_none=True)
        return out.detach().reshape(-1, 4).numpy().copy(), grads
    out, grads = _fp64(net, run)
    return act, G, out, grads


def _close(name, got, want):
    s = float(np.abs(want).max()) or 1.0
    err = float(np.abs(got - want).max()) / s
    assert err <= BAR, (name, err)
    return err


@pytest.mark.parametrize("d_hidden,beta", NETS)
def test_field_train_ref_matches_torch_float64(d_hidden, beta):
    net = net_for(d_hidden, beta)
    assert (net.mlp_coarse.n_blocks, net.mlp_coarse.combine_layer) == (N_BLOCKS, 2)
    xyz, vd, go = inputs_for(65)
    fwd, G, W = _reference(net, beta, xyz, vd, go)
    act_t, G_t, out_t, grads_t = _torch_layers(net, xyz, vd, go)
    worst = _close("out", fwd["out"], out_t)
    for l in range(2 * N_BLOCKS + 1):
        worst = max(worst, _close(f"act[{l}]", fwd["act"][l], act_t[l]), _close(f"G[{l}]", G[l], G_t[l]))
    for k in range(2 * N_BLOCKS):
        dW, db = FR.weight_grads(G[k], fwd["act"][k])
        name = f"blocks.{k // 2}.fc_{k % 2}"
        worst = max(worst, _close(name + ".weight", dW, grads_t[name + ".weight"]),
                    _close(name + ".bias", db, grads_t[name + ".bias"]))
    # the slope taken from the activation's value (the backward kernel's form) is the slope at the pre-activation
    for l in range(2 * N_BLOCKS + 1):
        a, b = FR.slope_of_act(fwd["act"][l], beta), FR.act_slope(fwd["pre"][l], beta)
        assert float(np.abs(a - b).max()) <= 1e-8     # torch's threshold: 1 where beta x > 20, 1 - e^-20 here
    print(f"field_train_ref vs torch float64, d_hidden {d_hidden} beta {beta}: worst {worst:.2e} (bar {BAR})")


@pytest.mark.parametrize("M", sorted({m for _, m in ROWS}))
@pytest.mark.parametrize("d_hidden,beta", [n for n in NETS if n[1] == 0.0])
def test_gpu_inputs_keep_the_relu_masks_decidable(d_hidden, beta, M):
    net = net_for(d_hidden, beta)
    fwd, _, _ = _reference(net, beta, *inputs_for(M))
    for l, pre in enumerate(fwd["pre"]):
        mx = float(np.abs(pre).max())
        assert not ((pre > 0) & (pre <= 2.0 ** -30 * mx)).any(), (l, "a pre-activation within 2^-30 of the layer max")
        for s in range(N_SCENES):
            for m0 in range(0, M, 64):
                wg = pre[s * M + m0:s * M + min(m0 + 64, M)]
                assert (wg > 0).any() and (wg <= 0).any(), (l, s, m0, "a workgroup's mask is all ones or all zeros")


@pytest.mark.parametrize("where", list(OUTLIER_ROWS))
@pytest.mark.parametrize("d_hidden,beta", sorted({(c[0], c[1]) for c in MAXIMA_LAYOUTS}))
def test_outlier_row_holds_every_layer_max(d_hidden, beta, where):
    net = net_for(d_hidden, beta)
    row = OUTLIER_ROWS[where]
    assert 0 <= row < N_SCENES * OUTLIER_M
    fwd, G, _ = _reference(net, beta, *outlier_inputs(row))
    for l in range(2 * N_BLOCKS + 1):
        assert int(np.abs(fwd["act"][l]).max(1).argmax()) == row, ("act", l)
        assert int(np.abs(G[l]).max(1).argmax()) == row, ("G", l)
        # by enough that the other rows alone would leave the split scale a factor 8 too large or more: fp16 infinities
        rest = np.delete(np.abs(G[l]).max(1), row)
        assert float(np.abs(G[l][row]).max()) >= 8 * float(rest.max()), ("G", l)
