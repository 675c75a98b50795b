"""Layer-by-layer HIP training of the ResnetFC options the fused training kernels do not carry: use_spade
(models.py:528-534, 585-587: before block b < combine_layer, x = scale_z[b](z) * x + lin_z[b](z)) and NS > 1
source views (models.py:566-579: block combine_layer starts from combine_interleaved, the mean or max over the
views, utils.py:71-81), alone or together, ReLU, no BatchNorm.

Both put an elementwise step between the fused kernels' 64-sample GEMM chains: the spade product needs the
interpolated scale rows, the combine mixes rows of different views (workgroups), so this path runs the MLP one
layer at a time on avr_bn_layer_run (the BatchNorm path's x3 layer GEMM over row-major fp32 rows, with identity
statistics: the operand is relu(x), the backward's mask [pre > 0]) with the elementwise steps between:
  forward   X[0] = lin_in(z_feature); per block b: (b < combine_layer) X'[b] = S_b * X[b] + T_b with T_b / S_b the
            bilinear blends of the per-texel lin_z / scale_z tables (avr_latent_features on the x3 tables: both
            carry their biases with use_spade, the product in torch; without it T_b has none, lin_z's bias is
            folded into the producing layer's bias and T_b is gathered in that layer's epilogue, avr_bn_layer's
            lin_z_table); (b == combine_layer, NS > 1) X'[b] = combine(X[b]) (torch); N[b] = fc_0(relu(X'[b]));
            X[b+1] = fc_1(relu(N[b])) + X'[b]; out = lin_out(relu(X[nb])), sigmoid / relu (avr_lin_out_fwd_rows).
  backward  lin_out and its activations (avr_lin_out_bwd_rows); the transposed layers on avr_bn_layer_run
            (W^T . g masked by [pre > 0]; fc_0^T adds the residual's g in its epilogue and publishes the max of
            what it stores), the spade product rule (d X = S * g, d S = g * X: avr_spade_bwd_rows; d T = g) and
            the combine's adjoint (the mean's in closed form, torch's for the max) between them; every weight
            gradient on avr_weight_grads (split-K x3; relu(X) rebuilt from the pre-activation rows in the
            staging), scale_z's against (g * X) rows; the latent / point gradients through the input functions
            as in avr.field._FieldTrain (the features' gradient on the lin_z^T layers where they apply).
"""
import torch

from . import _lib, ops, train_common as tc
from ._lib import stream_of
from .field import fused_eligible, softplus_beta, train_param_names, uses_bn
from .models import combine_interleaved
from .train_common import forward_train, gather_rows as _gather, lin_z_epilogue, padded_z_features

F32 = torch.float32


def layer_train_eligible(net):
    """A NewPixelNeRFNet this path trains: what the fused field runs for inference (avr.field.fused_eligible, with
    NS > 1 its multiview form), ReLU, no BatchNorm, and use_spade or NS > 1 source views (the other nets train on
    the fused kernels, avr.field._FieldTrain), d_latent a multiple of 64 up to 512 (x3 tables)."""
    try:
        mlps = [net.mlp_coarse] + ([net.mlp_fine] if net.mlp_fine is not None else [])
        ns = net.num_views_per_obj
        if any(uses_bn(m) or softplus_beta(m) != 0.0 for m in mlps):
            return False
        if not (ns > 1 or any(getattr(m, "use_spade", False) for m in mlps)):
            return False
        if not (net.d_latent % 64 == 0 and net.d_latent <= 512 and getattr(net, "field_precision", "x3") in ("x3", "fp16")):
            return False
        return fused_eligible(net, multiview=ns > 1, train=True)
    except AttributeError:
        return False


def train_param_names_layers(mlp):
    names = train_param_names(mlp)
    if getattr(mlp, "use_spade", False):
        for b in range(min(mlp.combine_layer, mlp.n_blocks)):
            names += [f"scale_z.{b}.weight", f"scale_z.{b}.bias"]
    return names


def forward_train_layers(fused, xyz, viewdirs, coarse):
    """The rf(xyz, viewdirs, coarse) protocol on this path (autograd when enabled)."""
    return forward_train(fused, xyz, viewdirs, coarse, _FieldTrainLayers, train_param_names_layers)


class _Ident:
    """Identity statistics: the BatchNorm layer kernels then compute relu(x) operands and [pre > 0] masks."""

    def __init__(self, H, dev):
        self.zero = torch.zeros(H, device=dev, dtype=F32)
        self.one = torch.ones(H, device=dev, dtype=F32)
        hidden = dict(in_dim=H, in_valid=H, ld_src=H)
        self._fields = {
            _lib.BN_FWD: dict(hidden, mode=_lib.BN_FWD, prologue=_lib.BN_RELU, in_mu=self.zero, in_scale=self.one,
                              in_shift=self.zero),
            _lib.BN_BWD: dict(hidden, mode=_lib.BN_BWD, prologue=_lib.BN_PLAIN, out_mu=self.zero, out_invstd=self.one,
                              out_scale=self.one, out_shift=self.zero)}

    def layer(self, mode, **kw):
        """The avr_bn_layer of a hidden (d_hidden x d_hidden) layer under these statistics: forward on the operand
        relu(src), backward W^T . src masked by [pre_rows > 0]; kw names what differs between the calls."""
        return tc.bn_layer(**self._fields[mode], **kw)


class _FieldTrainLayers(torch.autograd.Function):
    """Autograd of NewPixelNeRFNet.forward (models.py:739-863) for use_spade / NS > 1 nets, layer by layer (see the
    module docstring), for train.py's loss.backward() (train.py:108-114)."""

    @staticmethod
    def forward(ctx, fused, coarse, names, xyz, viewdirs, latent, *params):
        net = fused.net
        mlp = fused._mlp(coarse)
        P = dict(zip(names, params))
        entry = fused.packed(coarse)
        dims = entry.dims.with_precision(_lib.FIELD_X3)
        H, nb, nz = dims.d_hidden, dims.n_blocks, dims.n_lin_z
        spade = bool(dims.spade)
        NS = net.num_views_per_obj
        cl = mlp.combine_layer if NS > 1 else nb
        SB, B, _ = xyz.shape
        K = SB * NS
        M1, M2 = K * B, SB * B
        dev = xyz.device
        stream = stream_of(xyz)
        with torch.no_grad():
            p = xyz.detach().to(F32).repeat_interleave(NS, 0).contiguous()      # (object, view) rows
            zfp, d_in, zs = padded_z_features(net, xyz, viewdirs)                 # (M1, zs)
            tables = fused.tables_batch(coarse, K, fast=True)                     # (K, n_tables, HW, H)
            # without use_spade, X'[b] = X[b] + T_b: the T rows gathered in the epilogue of the layer producing X[b]
            # (avr_bn_layer's lin_z_table, as avr.bn_train; nz <= combine_layer, so X[b] is X'[b] and no T row is
            # stored); use_spade's product, or more scenes than one launch takes, gathers them here
            zk = not spade and 0 < nz and K <= _lib.AVR_MAX_SCENES
            views = fused.views(range(K), NS) if zk else None
            lin_z = lambda b: lin_z_epilogue(tables, b, nz, p, views, K, B) if zk else {}   # noqa: E731
            T = [] if zk else [_gather(fused, tables[:, b].contiguous(), K, NS, p, B, H) for b in range(nz)]
            S = [_gather(fused, tables[:, nz + b].contiguous(), K, NS, p, B, H) for b in range(nz)] if spade else []
            lz_b = [P[f"lin_z.{b}.bias"].detach().to(F32) for b in range(nz)]
            fold = (lambda b: 0) if spade else (lambda b: lz_b[b] if b < nz else 0)   # biases in the tables?
            b_in = (P["lin_in.bias"].detach().to(F32) + fold(0)).contiguous()
            b0 = [P[f"blocks.{b}.fc_0.bias"].detach().to(F32).contiguous() for b in range(nb)]
            b1 = [(P[f"blocks.{b}.fc_1.bias"].detach().to(F32) + fold(b + 1)).contiguous() for b in range(nb)]
            idt = _Ident(H, dev)
            part = tc.layer_partial(M1, H, dev)
            amax = torch.zeros(2 * nb, device=dev, dtype=torch.int32)
            blob = entry.packed
            rows = lambda b: M1 if b < cl else M2   # noqa: E731  (rows of block b)
            Xpre = [torch.empty(M1, H, device=dev, dtype=F32)]
            tc.run_layer(dims, tc.bn_layer(n_rows=M1, mode=_lib.BN_FWD, prologue=_lib.BN_PLAIN, in_dim=64,
                                           in_valid=d_in, src=zfp, ld_src=zs, blob=blob, layer=0, bias=b_in,
                                           out=Xpre[0], partial=part, **lin_z(0)), stream)
            Xin, N = [], []
            for b in range(nb):
                x = Xpre[b]
                if b < nz and not zk:                                       # models.py:583-588
                    x = torch.addcmul(T[b], S[b], x) if spade else x + T[b]
                if b == cl and NS > 1:
                    x = combine_interleaved(x, (NS, B), mlp.combine_type).reshape(M2, H)
                x = x.contiguous()
                Xin.append(x)
                m = rows(b)
                N.append(torch.empty(m, H, device=dev, dtype=F32))
                tc.run_layer(dims, idt.layer(_lib.BN_FWD, n_rows=m, src=x, operand_max=amax[2 * b:], blob=blob,
                                             layer=2 + 2 * b, bias=b0[b], out=N[b], partial=part), stream)
                Xpre.append(torch.empty(m, H, device=dev, dtype=F32))
                tc.run_layer(dims, idt.layer(_lib.BN_FWD, n_rows=m, src=N[b], operand_max=amax[2 * b + 1:], blob=blob,
                                             layer=3 + 2 * b, bias=b1[b], add1=x, out=Xpre[b + 1], partial=part,
                                             **lin_z(b + 1)), stream)
            # lin_out + sigmoid / relu in one pass (max relu(x) for its weight gradient; relu(x) not stored)
            out, a_max = ops.lin_out_rows(Xpre[nb], P["lin_out.weight"].detach(), P["lin_out.bias"].detach())
            out = out.reshape(SB, B, 4)
        ctx.fused, ctx.coarse, ctx.names, ctx.entry = fused, coarse, names, entry
        ctx.keep = (Xpre, Xin, N, S, amax, zfp, a_max, idt, p, cl)
        ctx.save_for_backward(xyz, viewdirs, latent, out, *params)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        xyz, viewdirs, latent, out, *params = ctx.saved_tensors
        Xpre, Xin, N, S, amax, zfp, a_max, idt, p, cl = ctx.keep
        ctx.keep = None
        fused, entry, names = ctx.fused, ctx.entry, ctx.names
        net = fused.net
        mlp = fused._mlp(ctx.coarse)
        P = dict(zip(names, params))
        dims = entry.dims.with_precision(_lib.FIELD_X3)
        H, nb, nz = dims.d_hidden, dims.n_blocks, dims.n_lin_z
        spade = bool(dims.spade)
        NS = net.num_views_per_obj
        SB, B, _ = xyz.shape
        K = SB * NS
        M1, M2 = K * B, SB * B
        dev = xyz.device
        stream = stream_of(xyz)
        want_latent = ctx.needs_input_grad[5] and not net.stop_encoder_grad
        want_xyz = ctx.needs_input_grad[3]
        with torch.no_grad():
            bwd = fused.packed_bwd(ctx.coarse, entry)
            part = tc.layer_partial(M1, H, dev)
            # the activations' backward (d4), lin_out^T and its relu's backward in one pass
            d4, g, d4_max = ops.lin_out_rows_bwd(grad_out.reshape(M2, 4), out.reshape(M2, 4),
                                                 P["lin_out.weight"].detach(), Xpre[nb])
            wl1, wl2 = [], []           # weight-gradient layers over M1 / M2 rows
            Gz, Gs, Gz_max, Gs_max = [None] * nz, [None] * nz, [None] * nz, [None] * nz
            blk = [None] * nb
            # max |operand| of every backward layer call, published by the layer kernels (the weight gradients'
            # scales for gp2 and g without a reduction pass over the rows): [2b] fc_0^T's, [2b + 1] fc_1^T's
            omax = torch.zeros(2 * nb, device=dev, dtype=torch.int32)
            relu_x = "relu"                                # X = relu(rows), rebuilt in the staging
            # max |stored rows| of each block's fc_0^T launch (ABI 14 out_max): Gz[b] for b < n_lin_z (<= the
            # combine layer, so no combine adjoint follows them), and g_in0 (lin_in's output gradient) unless
            # spade's product or the views' combine follows block 0's launch
            fc0t_max = torch.zeros(max(nb, 1), device=dev, dtype=torch.int32)
            in0_direct = nb > 0 and not spade and not (cl == 0 and NS > 1)
            for b in range(nb - 1, -1, -1):
                m = M1 if b < cl else M2
                # fc_1^T: gradient at N[b]; fc_0^T: the fc_0 path's gradient at X'[b]
                gp2 = torch.empty(m, H, device=dev, dtype=F32)
                tc.run_layer(dims, idt.layer(_lib.BN_BWD, n_rows=m, src=g, operand_max=omax[2 * b + 1:], blob=bwd,
                                             layer=3 + 2 * b, out=gp2, pre_rows=N[b], partial=part), stream)
                # fc_0^T, the residual's g added in its epilogue: d loss / d X'[b] (residual + fc_0 path)
                gin = torch.empty(m, H, device=dev, dtype=F32)
                tc.run_layer(dims, idt.layer(_lib.BN_BWD, n_rows=m, src=gp2, operand_max=omax[2 * b:], blob=bwd,
                                             layer=2 + 2 * b, out=gin, pre_rows=Xin[b], add1=g,
                                             out_max=fc0t_max[b:b + 1], partial=part), stream)
                blk[b] = [
                    (f"blocks.{b}.fc_0", (gp2, Xin[b], omax[2 * b:2 * b + 1], amax[2 * b:2 * b + 1], True, relu_x)),
                    (f"blocks.{b}.fc_1", (g, N[b], omax[2 * b + 1:2 * b + 2], amax[2 * b + 1:2 * b + 2], True, relu_x))]
                if b == cl and NS > 1 and mlp.combine_type == "average":
                    # the mean's adjoint (torch's MeanBackward: the gradient expanded over the views, / NS)
                    gin = (gin.reshape(SB, 1, B, H).expand(SB, NS, B, H) / NS).reshape(M1, H)   # one pass
                elif b == cl and NS > 1:                       # torch's adjoint of the views' combine
                    with torch.enable_grad():
                        xr = Xpre[b].detach().requires_grad_(True)
                        yc = combine_interleaved(xr, (NS, B), mlp.combine_type).reshape(M2, H)
                        gin, = torch.autograd.grad(yc, xr, gin)
                if b < nz:
                    Gz[b] = gin.contiguous()
                    Gz_max[b] = fc0t_max[b:b + 1]
                    if spade:                                  # X' = S * X + T (models.py:585-587)
                        # dS = g * X (+ its max for scale_z's weight gradient), dX = S * g: one pass
                        Gs[b], gin, Gs_max[b] = ops.spade_bwd_rows(Gz[b], Xpre[b].contiguous(), S[b])
                g = gin.contiguous()
            g_in0 = g                                          # d loss / d lin_in output
            for b in range(nb):
                (wl1 if b < cl else wl2).extend(blk[b])
            g_in0_max = fc0t_max[0:1] if in0_direct else ops._max_bits(g_in0)
            lat_feat = None
            if nz > 0:
                hwc = fused.latent_hwc_all(latent)
                if hwc.shape[0] != K:    # one map shared by the scenes (or more maps than scenes)
                    hwc = hwc[torch.clamp(torch.arange(K, device=dev), max=hwc.shape[0] - 1)].contiguous()
                lat_feat = _gather(fused, hwc, K, NS, p, B, net.d_latent)   # (lookup_features' batched launches)
                lat_max = fused.latent_max_bits(latent)
                for b in range(nz):
                    wl1.append((f"lin_z.{b}", (Gz[b], lat_feat, Gz_max[b], lat_max, True)))
                for b in range(nz if spade else 0):
                    wl1.append((f"scale_z.{b}", (Gs[b], lat_feat, Gs_max[b], lat_max, True)))
            wl1.append(("lin_in", (g_in0, zfp, g_in0_max, ops._max_bits(zfp), True)))
            wl2.append(("lin_out", (d4, Xpre[nb], d4_max, a_max, True, relu_x)))
            if M1 == M2:     # one source view: every layer over the same rows, one launch
                grads = tc.named_weight_grads(wl1 + wl2, M1, net.d_in)
            else:
                grads = {**tc.named_weight_grads(wl1, M1, net.d_in), **tc.named_weight_grads(wl2, M2, net.d_in)}
        g_feat = None
        # with stop_encoder_grad the looked-up latent is detached (models.py:810-811): no gradient reaches the
        # points through the lookup, z_feature's part alone (as avr.field._FieldTrain)
        if (want_latent or want_xyz) and nz > 0 and not net.stop_encoder_grad:
            if spade:
                pairs = [(Gz[b], P[f"lin_z.{b}.weight"].detach()) for b in range(nz)]
                pairs += [(Gs[b], P[f"scale_z.{b}.weight"].detach()) for b in range(nz)]
                g_feat = ops.sum_of_products(pairs)
            else:   # the lin_z^T layers on the x3 layer GEMM where they apply (train_common.feat_grad)
                g_feat = tc.feat_grad(fused, entry, bwd, Gz, P, M1)
        d_latent, d_xyz = tc.mlp_input_grads(fused, xyz, viewdirs, latent, want_latent, want_xyz, g_feat, g_in0,
                                             P["lin_in.weight"], NS)
        return tc.backward_result(ctx.needs_input_grad, names, grads, d_xyz, d_latent)
