"""What the three training Functions share (avr.field._FieldTrain, avr.bn_train._FieldTrainBN,
avr.layer_train._FieldTrainLayers): the rf(xyz, viewdirs, coarse) entry, the layer runner (avr_bn_layer_run) with
the feature gradient on its lin_z^T layers, the layer paths' padded z_feature operand and lin_z epilogue, the
weight gradients by parameter name, the interpolated-latent lookup, the input gradients -- the latent maps' through
the lookup's HIP adjoint (avr_latent_features_adjoint), the rest through torch autograd of net.mlp_inputs -- and
the backward's return tuple. Nothing here imports avr.field: a FusedField comes in as an argument. The Functions
call the runner through this module (train_common.run_layer), so a test or a diagnostic replaces it here."""
import ctypes
import os

import torch

from . import _lib, ops
from ._lib import BnLayer, call, ptr, scene_groups, size_query, stream_of

F32 = torch.float32


def bn_layer(**kw):
    """An avr_bn_layer from keyword fields (tensors become their device addresses)."""
    l = BnLayer()
    for k, v in kw.items():
        setattr(l, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return l


def run_layer(dims, layer, stream):
    call("avr_bn_layer_run", ctypes.byref(dims), ctypes.byref(layer), stream)


def layer_partial(M, H, dev):
    """The per-workgroup column partials of avr_bn_layer_run plus the fold scratch of avr_bn_stats."""
    return torch.empty(size_query("avr_bn_partial_floats", M, H), device=dev, dtype=F32)


def feat_grad(fused, entry, bwd, Gz, P, Mt):
    """The looked-up latent features' gradient sum_b Gz[b] . W_z[b] (the point / latent gradients' input):
    avr_bn_layer_run's lin_z[b]^T layers from the backward blob (x3, ABI 14), one launch per layer adding the
    previous layers' sum in its epilogue, where they apply (d_latent == d_hidden, ReLU, 64..512 wide); else
    fp32 library GEMMs (avr.ops.sum_of_products). entry: anything holding the blob's dims (an x3 copy is made)."""
    dims = entry.dims.with_precision(_lib.FIELD_X3)
    H, nz = dims.d_hidden, dims.n_lin_z
    if not (dims.d_latent == H and H in (64, 128, 256, 512) and not dims.spade and not dims.bn
            and not dims.beta > 0 and Mt > 0 and all(g.is_contiguous() for g in Gz)):
        return ops.sum_of_products([(Gz[b], P[f"lin_z.{b}.weight"].detach()) for b in range(nz)])
    dev = Gz[0].device
    part = layer_partial(Mt, H, dev)
    stream = stream_of(Gz[0])
    prev = None
    for b in range(nz):
        out = torch.empty(Mt, H, device=dev, dtype=F32)
        run_layer(dims, bn_layer(n_rows=Mt, mode=_lib.BN_BWD, prologue=_lib.BN_PLAIN, in_dim=H, in_valid=H, src=Gz[b],
                                 ld_src=H, blob=bwd, layer=_lib.BN_LAYER_LIN_Z_T + b, add1=prev, out=out,
                                 partial=part), stream)
        prev = out
    return prev


def forward_train(fused, xyz, viewdirs, coarse, function, param_names):
    """The rf(xyz, viewdirs, coarse) protocol with autograd on `function` (one of the three training Functions),
    differentiating the parameters param_names(mlp) names, in that order."""
    mlp = fused._mlp(coarse)
    names = param_names(mlp)
    named, _, _ = fused._state(mlp)
    return function.apply(fused, coarse, names, xyz, viewdirs, fused.net.encoder.latent, *[named[n] for n in names])


def padded_z_features(net, xyz, viewdirs):
    """lin_in's operand on the layer paths: net.z_features rows zero-padded to 16 B (the fused kernels' zf
    layout) -> (zfp (rows, zs), d_in, zs)."""
    zf = net.z_features(xyz.detach(), viewdirs.detach()).to(F32)
    d_in = zf.shape[1]
    zs = d_in + (-d_in) % 4
    zfp = torch.zeros(zf.shape[0], zs, device=zf.device, dtype=F32)
    zfp[:, :d_in] = zf
    return zfp, d_in, zs


def lin_z_epilogue(tables, b, nz, p, views, n_views, B):
    """avr_bn_layer fields adding lin_z[b](latent features) rows, gathered from the per-texel tables in the
    layer's epilogue (none past the last lin_z)."""
    if b >= nz:
        return {}
    return dict(lin_z_table=tables[0, b], lin_z_scene_stride=tables.stride(0), xyz=p,
                views=ctypes.addressof(views), n_views=n_views, rows_per_scene=B)


def named_weight_grads(named_layers, n_rows, d_in, specs_on=None):
    """One avr_weight_grads launch sequence over `named_layers`, (module name, layer) pairs in launch order (the
    order decides the chunking and, through the tile count, the K-split) -> {name + ".weight": dW, name + ".bias":
    db (None for a layer without want_bias)}. layer: an ops.weight_grads tuple, or with specs_on = (device, stream)
    an ops.weight_grads_specs integer spec. lin_in's operand rows are z_feature padded to 16 B: its dW keeps the
    first d_in columns."""
    layers = [layer for _, layer in named_layers]
    res = ops.weight_grads(layers, n_rows) if specs_on is None else ops.weight_grads_specs(layers, n_rows, *specs_on)
    grads = {}
    for (name, _), (dW, db) in zip(named_layers, res):
        grads[name + ".weight"], grads[name + ".bias"] = dW, db
    if "lin_in.weight" in grads:
        grads["lin_in.weight"] = grads["lin_in.weight"][:, :d_in].contiguous()
    return grads


def gather_rows(fused, tab, K, NS, p, B, C):
    """Bilinear blends (avr_latent_features' lookup and order) of the (K, H*W, C) per-texel rows `tab` at the
    points p (K, B, 3), scene k seen from source view k (object k // NS) -> (K * B, C); one launch per group."""
    out = torch.empty(K * B, C, device=p.device, dtype=F32)
    for g0, n in scene_groups(K):
        call("avr_latent_features_batch", fused.views(range(g0, g0 + n), NS), n, ptr(tab[g0]), C, ptr(p[g0]), B,
             ptr(out[g0 * B]), stream_of(out))
    return out


def lookup_features(fused, latent, p, n_scenes, B, ns=1):
    """The interpolated latent (grid_sample, models.py:266-273) at the points p (n_scenes, B, 3) ->
    (n_scenes * B, d_latent) row-major. Every scene its own map: gather_rows on the channels-last maps; fewer
    maps than scenes: scene by scene (avr_latent_features, the same kernel: the rows are bit-identical)."""
    C = latent.shape[1]
    if n_scenes <= latent.shape[0]:
        return gather_rows(fused, fused.latent_hwc_all(latent), n_scenes, ns, p, B, C)
    out = torch.empty(n_scenes * B, C, device=p.device, dtype=F32)
    for sb in range(n_scenes):
        s = min(sb, latent.shape[0] - 1)
        ops.latent_features(fused.view(sb, ns), latent[s], p[sb], out=out[sb * B:(sb + 1) * B],
                            hwc=fused.latent_hwc(latent, s))
    return out


def latent_grad_on_hip(latent, n_maps):
    """Whether d loss / d latent comes from the lookup's HIP adjoint (latent_grad_hip): an fp32 device map per
    (scene, view) -- one map shared by several scenes keeps the autograd path, which sums over them --, and not
    AVR_LATENT_GRAD_VIA_AUTOGRAD=1 (the earlier path, kept in the build for A/B). The callers' nets are
    fused_eligible (or its bn / layer equivalent): bilinear lookup, border padding."""
    return (latent.dtype == F32 and latent.is_cuda and latent.dim() == 4 and latent.shape[0] == n_maps
            and os.environ.get("AVR_LATENT_GRAD_VIA_AUTOGRAD") != "1")


def latent_grad_hip(fused, latent, xyz, g_feat, ns=1):
    """d loss / d latent (K, C, H, W), K = scenes * ns maps, from the looked-up features' gradient g_feat (K * B
    rows, or None: nothing passes through the lookup) on HIP: avr_latent_features_adjoint writes (K, H*W, C),
    returned as its (K, C, H, W) view (channels-last strides: no transpose pass; the encoder's backward takes it).
    Deterministic, unlike torch's grid_sampler_2d_backward (float atomics)."""
    K, C, H, W = latent.shape
    if g_feat is None:
        return torch.zeros_like(latent)
    with torch.no_grad():
        p = xyz.detach().to(F32)
        p = (p.repeat_interleave(ns, 0) if ns > 1 else p).contiguous()
        d_hwc = ops.latent_features_adjoint(fused.views(range(K), ns), p, g_feat, (H, W))
    return d_hwc.reshape(K, H, W, C).permute(0, 3, 1, 2)


def input_grads(fused, xyz, viewdirs, latent, want_latent, want_xyz, g_feat, g_zf, ns=1):
    """(d_latent, d_xyz) from the gradients at the MLP inputs (g_feat, g_zf as input_grads_via_autograd): the
    latent maps' on HIP where latent_grad_on_hip, whatever remains through torch autograd. Records which in
    fused.last_latent_grad ("hip" | "autograd") when the maps want a gradient."""
    d_latent = None
    if want_latent:
        hip = latent_grad_on_hip(latent, xyz.shape[0] * ns)
        fused.last_latent_grad = "hip" if hip else "autograd"
        if hip:
            d_latent, want_latent = latent_grad_hip(fused, latent, xyz, g_feat, ns), False
    d_lat, d_xyz = input_grads_via_autograd(fused.net, xyz, viewdirs, latent, want_latent, want_xyz, g_feat, g_zf)
    return (d_latent if d_latent is not None else d_lat), d_xyz


def input_grads_via_autograd(net, xyz, viewdirs, latent, want_latent, want_xyz, g_feat, g_zf):
    """(d_latent, d_xyz) from the gradients at the MLP inputs, sent through the (cheap) torch input functions
    net.mlp_inputs: the latent map via the grid_sample adjoint, the points via PE / rotation / projection.
    g_feat: the looked-up features' gradient, None when no gradient passes through the lookup (no lin_z, or
    stop_encoder_grad: the lookup is detached, models.py:810-811); g_zf: z_feature's (read with want_xyz)."""
    if not (want_latent or want_xyz):
        return None, None
    with torch.enable_grad():
        lat = latent.detach().requires_grad_(want_latent)
        x = xyz.detach().requires_grad_(want_xyz)
        feat, zft = net.mlp_inputs(x, viewdirs.detach(), latent=lat)
        outs, grads_out = [], []
        if g_feat is not None:
            outs.append(feat)
            grads_out.append(g_feat)
        if want_xyz:
            outs.append(zft)
            grads_out.append(g_zf)
        wrt = ([lat] if want_latent else []) + ([x] if want_xyz else [])
        res = torch.autograd.grad(outs, wrt, grads_out, allow_unused=True)
    d_latent = d_xyz = None
    if want_latent:
        d_latent = res[0] if res[0] is not None else torch.zeros_like(latent)
    if want_xyz:
        d_xyz = res[-1] if res[-1] is not None else torch.zeros_like(xyz)
    return d_latent, d_xyz


def mlp_input_grads(fused, xyz, viewdirs, latent, want_latent, want_xyz, g_feat, g_in0, w_in, ns=1):
    """(d_latent, d_xyz) as input_grads, from the gradient g_in0 at lin_in's output (z_feature's is g_in0 . w_in,
    formed when the points want one) and the looked-up features' g_feat, which each path forms its own way."""
    g_zf = g_in0 @ w_in.detach() if want_xyz else None
    return input_grads(fused, xyz, viewdirs, latent, want_latent, want_xyz, g_feat, g_zf, ns)


def backward_result(needs_input_grad, names, grads, d_xyz, d_latent):
    """A training Function's backward result for its inputs (fused, coarse, names, xyz, viewdirs, latent,
    *params): grads[name] for each parameter of `names` that wants a gradient."""
    return (None, None, None, d_xyz, None, d_latent) + tuple(
        grads[n] if needs_input_grad[6 + i] else None for i, n in enumerate(names))
