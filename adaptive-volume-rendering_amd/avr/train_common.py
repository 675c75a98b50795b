"""What the three training Functions share (avr.field._FieldTrain, avr.bn_train._FieldTrainBN,
avr.layer_train._FieldTrainLayers): the rf(xyz, viewdirs, coarse) entry, the layer paths' padded z_feature
operand and lin_z epilogue, the interpolated-latent lookup and the input gradients through torch autograd of
net.mlp_inputs. Nothing here imports avr.field: a FusedField comes in as an argument."""
import ctypes

import torch

from . import ops
from ._lib import call, ptr, scene_groups, stream_of

F32 = torch.float32


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
