"""Fused HIP evaluation of a NewPixelNeRFNet (models.py:739-863).

FusedField repacks each ResnetFC into MFMA fragment order (avr_field_pack),
projects the latent map through lin_z once per texel (avr_field_latent_table)
and evaluates sigma/RGB with one kernel launch per pass (avr_field_fwd_rays /
avr_field_fwd_points). Packed weights and tables are cached and rebuilt when a
parameter or the latent changes (tensor version counters), so an inference
loop over many frames of one scene pays for them once, as the reference pays
for encode() once.

Every cache entry goes through avr.cache's one protocol (_Record, _cached) under keys built from that module's
counters. A packed blob (_Packed) declares what hangs off it (backward blob, per-scene and batched lin_z tables) and
hands each library call a by-value copy of its dims for the kernel precision the call means (dims_as): the cached
struct is never written. _FieldTrain shares its entry, latent lookup and autograd tail with avr.bn_train /
avr.layer_train (avr.train_common).
"""
import ctypes
import operator
import os
import weakref

import torch

from . import _lib, ops, train_common
from ._lib import (FieldDims, ResnetFCWeights, ViewDesc, call, ptr, require_device, scene_groups, size_query,
                   stream_of)
from .cache import (_EXPLICIT_GEN, _MODULE_GEN, _PARAM_GEN, _Record, _cached, _hit, _slot_current, _stamp, _version_key,
                    bump_param_generation, param_generation)   # noqa: F401 (the last two: this module's API too)
from .train_common import feat_grad as _feat_grad, latent_grad_hip, latent_grad_on_hip, lookup_features

F32 = torch.float32
_blob = operator.attrgetter("packed")   # the device tensor of a _Packed: what its record's stamp marks


def uses_bn(mlp):
    """ResnetBlockFC(bn=True) blocks (train.py --bn, models.py:430-432, 456-461)."""
    return any(getattr(blk, "bn", False) for blk in getattr(mlp, "blocks", ()))


def softplus_beta(mlp):
    """beta of a ResnetFC(beta > 0) (models.py:442-445, 536-537: Softplus(beta) everywhere the
    ReLU would be), 0.0 for ReLU nets, None for anything else (torch's default threshold 20 only)."""
    acts = [mlp.activation] + [blk.activation for blk in mlp.blocks]
    if all(isinstance(a, torch.nn.ReLU) for a in acts):
        return 0.0
    if all(isinstance(a, torch.nn.Softplus) and a.threshold == 20 and a.beta > 0 for a in acts):
        betas = {float(a.beta) for a in acts}
        if len(betas) == 1:
            return betas.pop()
    return None


def inference_only(mlp):
    """ResnetFC options the fused x3 kernels run for inference only: BatchNorm (training mode trains layer by
    layer, avr.bn_train) and use_spade (module path). Softplus(beta) trains on the fused kernels (ABI 11)."""
    return uses_bn(mlp) or getattr(mlp, "use_spade", False)


def _bn_ok(blk):
    """Eval-mode BatchNorm with running statistics: a per-feature affine the
    x3 kernel applies (training-mode BN needs cross-sample statistics: module
    path)."""
    bn = blk.bn_0
    return (not blk.training and not bn.training and bn.track_running_stats and bn.running_mean is not None
            and bn.affine)


def _resnetfc_ok(mlp, d_in, d_latent, precision="x3"):
    if not (mlp is not None and type(mlp).__name__ == "ResnetFC" and getattr(mlp, "d_in", -1) == d_in
            and mlp.d_latent == d_latent and mlp.d_out == 4 and mlp.d_hidden in (64, 128, 256, 512)
            and 1 <= mlp.n_blocks <= _lib.AVR_MAX_BLOCKS and all(blk.shortcut is None for blk in mlp.blocks)):
        return False
    beta = softplus_beta(mlp)
    spade = getattr(mlp, "use_spade", False)
    bn = uses_bn(mlp)
    if beta is None or ((spade or beta > 0 or bn) and precision != "x3"):
        return False          # the fp32 kernel runs the default ReLU net only
    if bn and (spade or beta > 0):
        return False          # BatchNorm with use_spade / Softplus: module path
    return all(not blk.bn or _bn_ok(blk) for blk in mlp.blocks)


def fused_eligible(net, multiview=False, train=False):
    """True when `net` is a NewPixelNeRFNet configured like conf/default*.conf:
    local encoder, xyz + PE(xyz) + raw viewdirs, normalize_z, bilinear/border
    latent lookup, ResNet MLPs (eval-mode BatchNorm, use_spade and Softplus
    allowed on the x3 path), one source view. multiview: instead NS > 1 source
    views, x3, every MLP combining them (combine_layer < n_blocks, mean or max):
    FusedField.forward_points_multiview. train: for a call that needs gradients, where "fp16" (inference only)
    means what "x3" means."""
    try:
        ns = net.num_views_per_obj
        precision = getattr(net, "field_precision", "x3")
        if train:
            precision = blob_precision(precision)
        if multiview:
            mlps = [net.mlp_coarse] + ([net.mlp_fine] if net.mlp_fine is not None else [])
            if not (ns > 1 and precision == "x3"
                    and all(1 <= m.combine_layer < m.n_blocks and m.combine_type in ("average", "max")
                            for m in mlps)):
                # combine_layer 0 (views combined right after lin_in, no lin_z): module path -- the split
                # launch's first half needs at least one block (avr_field_fwd_points_split, b_end > 0)
                return False
        elif ns != 1:
            return False
        code = getattr(net, "code", None)
        enc = net.encoder
        ok = (net.use_encoder and net.use_xyz and net.normalize_z and net.use_code and net.use_viewdirs
              and not net.use_code_viewdirs and not getattr(net, "use_global_encoder", False)
              and code is not None and code.include_input and code.d_in == 3
              and getattr(enc, "index_interp", "bilinear") == "bilinear"
              and getattr(enc, "index_padding", "border") == "border"
              and enc.latent.dim() == 4 and enc.latent.shape[1] % 16 == 0 and enc.latent.shape[1] <= 1024
              and net.d_in == 6 * code.num_freqs + 6)
        if not ok:
            return False
        mlps = [net.mlp_coarse] + ([net.mlp_fine] if net.mlp_fine is not None else [])
        return all(_resnetfc_ok(m, net.d_in, net.d_latent, precision) for m in mlps)
    except AttributeError:
        return False


def _freq_factor(code):
    ff = getattr(code, "freq_factor", None)
    if ff is None:
        ff = float(code.freqs[0])
    return float(ff)


PRECISIONS = {"fp32": _lib.FIELD_FP32, "x3": _lib.FIELD_X3, "fp16": _lib.FIELD_FP16}


def blob_precision(precision):
    """The precision a blob is packed and cached under: "fp16" reads the x3 blob byte for byte (its hi halves),
    so the two share one _Packed record and one set of lin_z tables; "fp32" has its own."""
    return "x3" if precision == "fp16" else precision


class _Packed:
    """One packed ResnetFC: dims (the struct avr_field_pack was called with) and the blob, the weight pointers
    with the tensors behind them, and what is derived from the blob and dies with it: the backward blob (a
    _Record or None), the per-scene lin_z tables (sb -> _Record) and the batched ones (fast -> _Record)."""

    def __init__(self, dims, packed, weights=None, keep=None):
        self.dims = dims
        self.packed = packed
        self.weights = weights
        self.keep = keep
        self.bwd = None
        self.tables = {}
        self.batch_tables = {}
        self._dims_as = {precision: dims.with_precision(precision) for precision in PRECISIONS.values()}

    def dims_as(self, precision):
        """A copy of dims selecting the `precision` kernels (_lib.FIELD_X3 / FIELD_FP32 / FIELD_FP16): what a library
        call is given, so that dims itself keeps describing the blob."""
        return self._dims_as[precision]


def n_tables(dims):
    """Per-texel tables of a packed net: lin_z[b], then scale_z[b] with use_spade."""
    return dims.n_lin_z * (2 if dims.spade else 1)


class FusedField:
    """precision: "x3" (default) = split-fp16 MFMA (3 products per fp32 product,
    fp32 accumulation, within fp32 noise of the fp32 path); "fp32" = fp32 MFMA;
    "fp16" = one fp16 product per term on the x3 blob (inference only, ~1e-4 mean rgb
    error: for 8-bit frames; ReLU nets, one source view; training calls run x3)."""

    def __init__(self, net, precision="x3"):
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
        self.precision = precision
        self.net = net
        # how the last training backward formed d loss / d latent: "hip" (avr_latent_features_adjoint) | "autograd"
        # (torch's grid_sample adjoint), None before the first (for tests / introspection, as renderers' last_path)
        self.last_latent_grad = None
        # the caches: slot -> _Record, read and filled by _cached
        self._packed = {}         # coarse, or (coarse, "bn_train") -> _Record of a _Packed (tables hang off it)
        self._view_cache = {}     # (sb, ns) -> ViewDesc (view()); (range, ns) -> ViewDesc arrays (views())
        self._latent_cache = {}   # per latent version: channels-last copies, max |latent| (both MLPs share them)
        self._pack_args = {}      # slot of _packed -> the last build's _pack_weights(), reused while the pointers stay
        # mlp (weakly) -> ([(name, owner dict, key)] params, [...] float buffers, generation, ids of its modules)
        self._slots = weakref.WeakKeyDictionary()

    def invalidate(self, views=True):
        """Drop every cached blob, table and (views=True) view descriptor (avr.parallel.broadcast_scene calls it
        after writing a scene into the net; the (data_ptr, _version) keys would catch that too). views=False keeps
        the host-side view descriptors (avr.graphs.GraphedTrainStep before a capture: building one reads the poses
        back to the host, which a capture cannot do)."""
        self._packed.clear()
        self._pack_args.clear()
        if views:
            self._view_cache.clear()
        self._latent_cache.clear()

    def cache_tensors(self):
        """Every device buffer the caches hold (packed blobs, backward blobs, lin_z tables, batched tables):
        what a captured HIP graph reads (avr.graphs.GraphedRenderer keeps references to them, so an eager call
        that replaces a cache entry cannot free memory a replay still reads)."""
        out = []
        for entry in (rec[1] for rec in self._packed.values() if rec[1] is not None):
            recs = [entry.bwd, *entry.tables.values(), *entry.batch_tables.values()]
            out += [entry.packed] + [r.value for r in recs if r is not None]
        return out

    def _latent_cached(self, what, latent, make):
        # the optimizer-step count matters only for a latent an optimizer can hold: a leaf that requires grad, or a
        # view of one (param[idx] shares the leaf's storage, which a fused optimizer updates past every version
        # counter). A fixed or encoder-produced map keeps its copies across steps (in-place writes advance its version)
        held = any(t is not None and t.is_leaf and t.requires_grad for t in (latent, latent._base))
        gen = _PARAM_GEN[0] if held else (-1, _EXPLICIT_GEN[0])
        key = (gen, latent.data_ptr(), latent._version, tuple(latent.shape))
        return _cached(self._latent_cache, what, key, make, keep=latent)   # held: its address is in the key

    def latent_hwc(self, latent, s):
        """Scene s's latent map channels-last (avr_latent_features' operand), once per latent version."""
        return self._latent_cached(("hwc", s), latent, lambda: ops.latent_hwc(latent[s]))

    def latent_hwc_all(self, latent):
        """Every scene's latent map channels-last, (SB, H*W, C), once per latent version."""
        def make():
            SB, C, H, W = latent.shape
            return latent.detach().to(F32).reshape(SB, C, H * W).transpose(1, 2).contiguous()
        return self._latent_cached("hwc_all", latent, make)

    def latent_max_bits(self, latent):
        """max |latent| as int32 float bits (the lin_z weight gradients' X scale), once per latent version."""
        return self._latent_cached("max", latent, lambda: ops._max_bits(latent))

    # ----------------------------------------------------------- parameters
    def _state(self, mlp):
        """(named parameters, parameters, floating-point buffers) of mlp in named_parameters() / buffers() order,
        read through each owning module's dict: the module tree is walked once per mlp and again after any
        submodule registration (a walk per call was a large part of the adaptive step's host time), and a
        parameter or buffer replaced later is still seen."""
        hit = self._slots.get(mlp)
        if hit is not None and hit[2] != _MODULE_GEN[0]:
            hit = (hit[0], hit[1], _MODULE_GEN[0], hit[3]) if _slot_current(hit[2], hit[3]) else None
            if hit is not None:
                self._slots[mlp] = hit
        if hit is None:
            mods = list(mlp.named_modules())
            ps = [(f"{mn}.{n}" if mn else n, m._parameters, n) for mn, m in mods
                  for n, t in m._parameters.items() if t is not None]
            bs = [(f"{mn}.{n}" if mn else n, m._buffers, n) for mn, m in mods
                  for n, t in m._buffers.items() if t is not None and t.is_floating_point()]
            hit = (ps, bs, _MODULE_GEN[0], frozenset(id(m) for _, m in mods))
            self._slots[mlp] = hit
        named = {full: d[k] for full, d, k in hit[0]}
        return named, list(named.values()), [d[k] for _, d, k in hit[1]]

    def _mlp(self, coarse):
        net = self.net
        return net.mlp_coarse if (coarse or net.mlp_fine is None) else net.mlp_fine

    def dims(self, mlp):
        code = self.net.code
        return FieldDims(self.net.d_in, self.net.d_latent, mlp.d_hidden, mlp.n_blocks,
                         min(mlp.combine_layer, mlp.n_blocks), code.num_freqs, _freq_factor(code),
                         PRECISIONS[blob_precision(self.precision)], int(uses_bn(mlp)),
                         int(getattr(mlp, "use_spade", False)),
                         float(softplus_beta(mlp) or 0.0))

    def packed(self, coarse, bn_fold=True):
        """bn_fold=False: the training-mode BatchNorm path's blob (avr.bn_train): x3, raw fc_0 weights (no
        eval-BN folding, dims.bn = 0), cached beside the inference blob."""
        mlp = self._mlp(coarse)
        _, ps, bs = self._state(mlp)
        params = ps + bs
        # the precision is part of the key: an x3 blob holds only the fragments the x3 kernels read
        # (avr_field_pack), and net.fused() switches a FusedField's precision in place
        slot = coarse if bn_fold else (coarse, "bn_train")
        key = (id(mlp), blob_precision(self.precision) if bn_fold else "x3", _version_key(params))

        def make():
            dims = self.dims(mlp)
            if not bn_fold:
                dims.bn, dims.precision = 0, _lib.FIELD_X3
            # an optimizer step updates the parameters in place: same tensors, same addresses, so the last build's
            # weight pointers, blob size and kept tensors serve again and only the pack launch reruns (when every
            # pointer was a parameter or buffer read in place; derived tensors -- BN folds, conversions -- are rebuilt)
            args_key = (id(mlp), tuple(pv[0] for pv in key[2][1:]), bytes(dims))
            n, w, keep, in_place = _cached(self._pack_args, slot, args_key, lambda: self._pack_weights(mlp, dims),
                                           device=False)
            if not in_place:
                del self._pack_args[slot]
            packed = torch.empty(n, device=params[0].device, dtype=F32)
            call("avr_field_pack", ctypes.byref(dims), ctypes.byref(w), ptr(packed), stream_of(packed))
            return _Packed(dims, packed, w, keep)
        return _cached(self._packed, slot, key, make, of=_blob)

    def _pack_weights(self, mlp, dims):
        """avr_field_pack's arguments for mlp: (blob floats, weight pointers, the tensors behind them, whether every
        pointer is a parameter or buffer read in place)."""
        n = size_query("avr_field_packed_floats", ctypes.byref(dims))
        w = ResnetFCWeights()
        keep = []
        derived = [False]

        def P(t):
            if not (t.dtype == F32 and t.is_contiguous()):   # (fp32 contiguous parameters: read in place)
                t = t.detach().to(F32).contiguous()
                derived[0] = True
            keep.append(t)
            return t.data_ptr()

        w.lin_in_w, w.lin_in_b = P(mlp.lin_in.weight), P(mlp.lin_in.bias)
        w.lin_out_w, w.lin_out_b = P(mlp.lin_out.weight), P(mlp.lin_out.bias)
        for b, blk in enumerate(mlp.blocks):
            if dims.bn:
                # eval BatchNorm1d as y = a x + c (torch's batch_norm: a = w / sqrt(var + eps), c = b - mean a);
                # bn_0 sits in front of both relus of the block (models.py:456-461): the first is applied by
                # the kernel, the second folds into fc_0's rows
                bn = blk.bn_0
                a = (bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps))
                c = bn.bias.detach().float() - bn.running_mean.detach().float() * a
                w.bn_scale[b], w.bn_shift[b] = P(a), P(c)
                w.fc0_w[b] = P(blk.fc_0.weight.detach().float() * a[:, None])
                w.fc0_b[b] = P(blk.fc_0.bias.detach().float() * a + c)
            else:
                w.fc0_w[b], w.fc0_b[b] = P(blk.fc_0.weight), P(blk.fc_0.bias)
            w.fc1_w[b], w.fc1_b[b] = P(blk.fc_1.weight), P(blk.fc_1.bias)
        for b in range(dims.n_lin_z):
            w.lin_z_w[b], w.lin_z_b[b] = P(mlp.lin_z[b].weight), P(mlp.lin_z[b].bias)
            if dims.spade:   # scale_z[b](z) * x + lin_z[b](z) (models.py:585-587): both as per-texel tables
                w.scale_z_w[b], w.scale_z_b[b] = P(mlp.scale_z[b].weight), P(mlp.scale_z[b].bias)
        require_device(*keep)
        return n, w, keep, not (dims.bn or derived[0])

    def packed_bwd(self, coarse, entry=None):
        """Transposed fc_0 / fc_1 fragments for the backward kernel, cached with
        the forward blob (rebuilt whenever a parameter changes)."""
        entry = entry or self.packed(coarse)
        if not _hit(entry.bwd, None):
            dims = entry.dims_as(_lib.FIELD_X3)   # (the backward blob is x3 fragments; the C side reads no precision)
            n = size_query("avr_field_bwd_packed_floats", ctypes.byref(dims))
            bwd = torch.empty(n, device=entry.packed.device, dtype=F32)
            call("avr_field_pack_bwd", ctypes.byref(dims), ctypes.byref(entry.weights), ptr(bwd), stream_of(bwd))
            entry.bwd = _Record(None, bwd, None, _stamp(bwd))
        return entry.bwd.value

    def table(self, coarse, sb=0):
        entry = self.packed(coarse)
        lat = self.net.encoder.latent
        key = (sb, _PARAM_GEN[0], lat.data_ptr(), lat._version, tuple(lat.shape))

        def make():
            dims = entry.dims_as(_lib.FIELD_FP32)   # inference: exact fp32 tables, computed once per latent map
            L, H, W = lat.shape[1:]
            latent = lat[sb].detach().to(F32).contiguous()
            require_device(latent)
            table = torch.empty(max(n_tables(dims), 1), H * W, dims.d_hidden, device=latent.device, dtype=F32)
            call("avr_field_latent_table", ctypes.byref(dims), ptr(entry.packed), ptr(latent), H, W, ptr(table),
                 stream_of(table))
            return table
        return _cached(entry.tables, sb, key, make, keep=lat)   # holding `lat` keeps its address from being reused

    def tables_batch(self, coarse, n_scenes, fast=False, bn_fold=True, entry=None):
        """The lin_z tables of scenes 0 .. n_scenes-1 back to back, (n_scenes,
        max(n_tables, 1), H*W, d_hidden): one buffer for the multi-scene launches.
        fast (the training path, which recomputes them every step): on the split-fp16
        GEMM (table_x3_kernel); otherwise exact fp32 products. bn_fold: which blob's
        cache holds them (packed()); entry: that packed() result when the caller has it."""
        entry = entry or self.packed(coarse, bn_fold)
        lat = self.net.encoder.latent
        key = (n_scenes, bool(fast), _PARAM_GEN[0], lat.data_ptr(), lat._version, tuple(lat.shape))

        def make():
            dims = entry.dims_as(_lib.FIELD_X3 if fast else _lib.FIELD_FP32)
            L, H, W = lat.shape[1:]
            out = torch.empty(n_scenes, max(n_tables(dims), 1), H * W, dims.d_hidden, device=lat.device, dtype=F32)
            if n_scenes <= lat.shape[0]:   # every scene its own map: one launch
                latent = lat[:n_scenes].detach().to(F32).contiguous()
                call("avr_field_latent_table_batch", ctypes.byref(dims), ptr(entry.packed), ptr(latent), n_scenes,
                     H, W, ptr(out), stream_of(out))
            else:
                for sb in range(n_scenes):
                    latent = lat[min(sb, lat.shape[0] - 1)].detach().to(F32).contiguous()
                    call("avr_field_latent_table", ctypes.byref(dims), ptr(entry.packed), ptr(latent), H, W,
                         ptr(out[sb]), stream_of(out))
            return out
        return _cached(entry.batch_tables, bool(fast), key, make, keep=lat)

    def _view_sources(self):
        """The tensors a ViewDesc is read from (a view cache entry holds them: its (ptr, version) key stays sound)."""
        net = self.net
        return [net.poses, net.focal, net.c, net.image_shape, net.encoder.latent_scaling]

    def view(self, sb=0, ns=1):
        """Source view sb (pose sb; with ns > 1 views per object, focal / principal point of
        object sb // ns, as models.py:796-801 repeat_interleaves them)."""
        net = self.net
        srcs = self._view_sources()
        key = (sb, ns, _version_key(srcs, gen=False), tuple(net.encoder.latent.shape))

        def make():
            pick = lambda t, i=sb: t[min(i, t.shape[0] - 1)] if t.dim() > 1 else t  # noqa: E731
            v = ViewDesc()
            v.poses[:] = [float(x) for x in pick(net.poses).reshape(-1)[:12].tolist()]
            v.focal[:] = [float(x) for x in pick(net.focal, sb // ns).reshape(-1)[:2].tolist()]
            v.c[:] = [float(x) for x in pick(net.c, sb // ns).reshape(-1)[:2].tolist()]
            v.image_shape[:] = [float(x) for x in net.image_shape.reshape(-1)[:2].tolist()]
            v.latent_scaling[:] = [float(x) for x in net.encoder.latent_scaling.reshape(-1)[:2].tolist()]
            v.latent_h, v.latent_w = int(net.encoder.latent.shape[-2]), int(net.encoder.latent.shape[-1])
            return v
        return _cached(self._view_cache, (sb, ns), key, make, keep=srcs, device=False)

    def views(self, idx, ns=1):
        """The ViewDesc array of view(i, ns) for i in the range idx (the multi-scene launches' argument), cached
        under one source-version key (per-view keys for every scene of every launch were host time)."""
        srcs = self._view_sources()
        key = (_version_key(srcs, gen=False), tuple(self.net.encoder.latent.shape))
        return _cached(self._view_cache, (idx.start, idx.stop, idx.step, ns), key,
                       lambda: (ViewDesc * len(idx))(*[self.view(i, ns) for i in idx]), keep=srcs, device=False)

    # ----------------------------------------------------------- evaluation
    def forward_rays(self, ro, rd, z, coarse, sb=0):
        """sigma/RGB at ro[r] + rd[r]*z[r,s] with viewdir rd[r]: (R*N, 4)."""
        R, N = z.shape
        ro = ro.reshape(R, 3).to(F32).contiguous()
        rd = rd.reshape(R, 3).to(F32).contiguous()
        z = z.to(F32).contiguous()
        require_device(ro, rd, z)
        entry = self.packed(coarse)
        table = self.table(coarse, sb)
        out = torch.empty(R * N, 4, device=z.device, dtype=F32)
        dims = entry.dims_as(PRECISIONS[self.precision])
        call("avr_field_fwd_rays", ctypes.byref(dims), ctypes.byref(self.view(sb)), ptr(entry.packed),
             ptr(table), ptr(ro), ptr(rd), ptr(z), R, N, ptr(out), stream_of(z))
        return out

    def forward_rays_batch(self, ro, rd, z, coarse):
        """SB scenes at once: ro, rd (SB, R, 3), z (SB*R, N) -> (SB*R*N, 4); one x3
        launch per group of up to AVR_MAX_SCENES scenes (avr_field_fwd_rays_batch)."""
        SB, R, _ = ro.shape
        N = z.shape[-1]
        ro = ro.to(F32).contiguous()
        rd = rd.to(F32).contiguous()
        z = z.to(F32).reshape(SB * R, N).contiguous()
        require_device(ro, rd, z)
        out = torch.empty(SB * R * N, 4, device=z.device, dtype=F32)
        if self.precision == "fp32":     # the fp32 kernel is single-scene
            for b in range(SB):
                out[b * R * N:(b + 1) * R * N] = self.forward_rays(ro[b], rd[b], z[b * R:(b + 1) * R], coarse, sb=b)
            return out
        entry = self.packed(coarse)
        tables = self.tables_batch(coarse, SB)
        dims = entry.dims_as(PRECISIONS[self.precision])
        for g0, n in scene_groups(SB):
            views = self.views(range(g0, g0 + n))
            call("avr_field_fwd_rays_batch", ctypes.byref(dims), views, n, ptr(entry.packed), ptr(tables[g0]),
                 ptr(ro[g0]), ptr(rd[g0]), ptr(z[g0 * R]), R, N, ptr(out[g0 * R * N]), stream_of(z))
        return out

    def forward_points_multiview(self, xyz, viewdirs, coarse):
        """NS = net.num_views_per_obj > 1 source views per object (models.py:749-853): the MLP's
        first combine_layer blocks run on every (object, view) pair (avr_field_fwd_points_split,
        first launch), the residual streams are combined over the views exactly as ResnetFC does
        (combine_interleaved, models.py:566-579 / utils.py:71-81: mean or max over NS), and the
        remaining blocks + lin_out run once per object (second launch). (SB, B, 3) -> (SB, B, 4)."""
        from .models import combine_interleaved
        net = self.net
        NS = net.num_views_per_obj
        SB, B, _ = xyz.shape
        mlp = self._mlp(coarse)
        entry = self.packed(coarse)
        dims = entry.dims_as(_lib.FIELD_X3)
        H, nb, cl = dims.d_hidden, dims.n_blocks, mlp.combine_layer
        dev = xyz.device
        p = xyz.to(F32).repeat_interleave(NS, 0).contiguous()              # (SB*NS, B, 3), views of an object adjacent
        v = viewdirs.reshape(SB, B, 3).to(F32).repeat_interleave(NS, 0).contiguous()
        require_device(p, v)
        K = SB * NS
        tables = self.tables_batch(coarse, K)
        h = torch.empty(K * B, H, device=dev, dtype=F32)
        out = torch.empty(SB, B, 4, device=dev, dtype=F32)
        for g0, n in scene_groups(K):
            views = self.views(range(g0, g0 + n), NS)
            call("avr_field_fwd_points_split", ctypes.byref(dims), views, n, ptr(entry.packed),
                 ptr(tables[g0]), ptr(p[g0]), ptr(v[g0]), B, 0, cl, None, ptr(h[g0 * B]), None, stream_of(p))
        hc = combine_interleaved(h, (NS, B), mlp.combine_type).reshape(SB * B, H).contiguous()
        for g0, n in scene_groups(SB):
            views = self.views(range(g0 * NS, (g0 + n) * NS, NS), NS)
            call("avr_field_fwd_points_split", ctypes.byref(dims), views, n, ptr(entry.packed),
                 ptr(tables[0]), None, None, B, cl, nb, ptr(hc[g0 * B]), None, ptr(out[g0]), stream_of(p))
        return out

    def forward_points(self, xyz, viewdirs, coarse):
        """The rf(xyz (SB,B,3), viewdirs, coarse) protocol -> (SB, B, 4)."""
        if getattr(self.net, "num_views_per_obj", 1) > 1:
            # NS > 1 runs on the x3 split launches only: another precision or an ineligible combine must not be
            # served silently at x3
            if self.precision != "x3" or not fused_eligible(self.net, multiview=True):
                raise _lib.AVRError("FusedField.forward_points: NS > 1 source views need precision 'x3' and an "
                                    "eligible combine (1 <= combine_layer < n_blocks); use the module path")
            return self.forward_points_multiview(xyz, viewdirs, coarse)
        SB, B, _ = xyz.shape
        out = torch.empty(SB, B, 4, device=xyz.device, dtype=F32)
        entry = self.packed(coarse)
        if SB > 1 and self.precision != "fp32":   # one launch per group of scenes
            p = xyz.to(F32).contiguous()
            v = viewdirs.reshape(SB, B, 3).to(F32).contiguous()
            require_device(p, v)
            tables = self.tables_batch(coarse, SB)
            dims = entry.dims_as(PRECISIONS[self.precision])
            for g0, n in scene_groups(SB):
                views = self.views(range(g0, g0 + n))
                call("avr_field_fwd_points_batch", ctypes.byref(dims), views, n, ptr(entry.packed),
                     ptr(tables[g0]), ptr(p[g0]), ptr(v[g0]), B, ptr(out[g0]), stream_of(p))
            return out
        for sb in range(SB):
            self.forward_points_scene(xyz[sb], viewdirs.reshape(SB, B, 3)[sb], coarse, sb, out=out[sb])
        return out

    def forward_points_scene(self, xyz, viewdirs, coarse, sb=0, out=None):
        """Scene sb's field at a point list: xyz, viewdirs (M, 3) -> (M, 4), one avr_field_fwd_points launch with
        that scene's view and lin_z tables (single-view nets)."""
        M = xyz.shape[0]
        p = xyz.to(F32).contiguous()
        v = viewdirs.to(F32).contiguous()
        require_device(p, v)
        if out is None:
            out = torch.empty(M, 4, device=p.device, dtype=F32)
        entry = self.packed(coarse)
        dims = entry.dims_as(PRECISIONS[self.precision])
        table = self.table(coarse, sb)
        call("avr_field_fwd_points", ctypes.byref(dims), ctypes.byref(self.view(sb)), ptr(entry.packed),
             ptr(table), ptr(p), ptr(v), M, ptr(out), stream_of(p))
        return out

    def forward_points_scene_counted(self, xyz, viewdirs, n_points, coarse, sb=0, out=None):
        """forward_points_scene over the first n_points rows of xyz, viewdirs (capacity, 3), n_points a 0-dim int64
        tensor on the device (avr_field_fwd_points_counted): rows at or beyond it are neither read nor written, no
        host read sizes the launch. -> (capacity, 4). ReLU nets without BatchNorm or use_spade: the other inference
        variants have no counted kernel and raise ValueError (never another path)."""
        cap = xyz.shape[0]
        if xyz.dtype != F32 or viewdirs.dtype != F32 or not (xyz.is_contiguous() and viewdirs.is_contiguous()):
            raise ValueError("forward_points_scene_counted: xyz and viewdirs must be contiguous fp32 (a conversion "
                             "would read the rows beyond the count)")
        if n_points.dtype != torch.int64 or n_points.numel() != 1:
            raise ValueError("forward_points_scene_counted: n_points must be one int64 on the device")
        require_device(xyz, viewdirs)
        if not n_points.is_cuda:
            raise ValueError("forward_points_scene_counted: n_points must be on the device")
        entry = self.packed(coarse)
        dims = entry.dims_as(PRECISIONS[self.precision])
        if dims.bn or dims.spade or dims.beta > 0:
            raise ValueError("device-count occupancy gating (occupancy_count = 'device') has counted field kernels "
                             "for ReLU nets without BatchNorm or use_spade only; use occupancy_count = 'host'")
        if out is None:
            out = torch.empty(cap, 4, device=xyz.device, dtype=F32)
        table = self.table(coarse, sb)
        call("avr_field_fwd_points_counted", ctypes.byref(dims), ctypes.byref(self.view(sb)), ptr(entry.packed),
             ptr(table), ptr(xyz), ptr(viewdirs), cap, ptr(n_points), ptr(out), stream_of(xyz))
        return out

    # ----------------------------------------------------------- training
    def forward_train(self, xyz, viewdirs, coarse):
        """The rf(xyz, viewdirs, coarse) protocol with autograd: HIP forward that
        keeps every GEMM input, HIP backward through the ResnetFC, weight
        gradients as GEMMs over the samples (see _FieldTrain)."""
        return train_common.forward_train(self, xyz, viewdirs, coarse, _FieldTrain, train_param_names)


def train_param_names(mlp):
    """The ResnetFC parameters the training path differentiates, in a fixed order."""
    names = ["lin_in.weight", "lin_in.bias", "lin_out.weight", "lin_out.bias"]
    for b in range(mlp.n_blocks):
        names += [f"blocks.{b}.fc_0.weight", f"blocks.{b}.fc_0.bias", f"blocks.{b}.fc_1.weight", f"blocks.{b}.fc_1.bias"]
    for b in range(min(mlp.combine_layer, mlp.n_blocks)):
        names += [f"lin_z.{b}.weight", f"lin_z.{b}.bias"]
    return names


def _bwd_chain(dims, entry, bwd, masks, B, Mt, out, grad_out, act):
    """avr_field_bwd per group of scenes: the gradient at every layer output, (layers, Mt, d_hidden), and each
    layer's max |gradient| as int32 float bits."""
    H, n_l = dims.d_hidden, 2 * dims.n_blocks + 1
    G = torch.empty(n_l, Mt, H, device=out.device, dtype=F32)
    g_max = torch.zeros(n_l, device=out.device, dtype=torch.int32)
    for g0, n, mask in masks:
        call("avr_field_bwd", ctypes.byref(dims), ptr(entry.packed), ptr(bwd), n, B, ptr(out[g0]),
             ptr(grad_out[g0]), ptr(mask), ptr(act, g0 * B * H), Mt, ptr(G, g0 * B * H), Mt, ptr(g_max),
             stream_of(G))
    return G, g_max


def _weight_grads(dims, Mt, G, g_max, act, act_max, lat_feat, lat_max, zf, d4, d4_max):
    """Every weight and bias gradient by parameter name, from one batched avr_weight_grads launch. Its layers are
    addressed by offset into the buffers _FieldTrain allocated (row strides H, d_latent, zs, 4; 16-B aligned by
    construction): the fc layers (G_k, act_k), lin_z[b] (the gradient at block b's input, the interpolated
    latent), lin_in (the gradient at the first block's input, z_feature with its max in act_max[n_l]), lin_out
    (d4, the last block's output) -- no per-layer views or checks."""
    H, nb, nz, d_latent = dims.d_hidden, dims.n_blocks, dims.n_lin_z, dims.d_latent
    Gp, Ap, gmp, amp, lay = G.data_ptr(), act.data_ptr(), g_max.data_ptr(), act_max.data_ptr(), Mt * H * 4
    layers = [(f"blocks.{k // 2}.fc_{k % 2}",
               (Gp + k * lay, H, Ap + k * lay, H, H, H, gmp + 4 * k, amp + 4 * k, True, None, None, None, 0))
              for k in range(2 * nb)]
    for b in range(nz):
        k = 2 * b - 1 if b > 0 else 2 * nb
        layers.append((f"lin_z.{b}", (Gp + k * lay, H, lat_feat.data_ptr(), d_latent, H, d_latent, gmp + 4 * k,
                                      lat_max.data_ptr(), False, None, None, None, 0)))
    layers.append(("lin_in", (Gp + 2 * nb * lay, H, zf.data_ptr(), zf.shape[1], H, zf.shape[1], gmp + 8 * nb,
                              amp + 4 * (2 * nb + 1), True, None, None, None, 0)))
    layers.append(("lin_out", (d4.data_ptr(), 4, Ap + 2 * nb * lay, H, 4, H, d4_max.data_ptr(), amp + 8 * nb, True,
                               None, None, None, 0)))
    grads = train_common.named_weight_grads(layers, Mt, dims.d_in, specs_on=(G.device, stream_of(G)))
    for b in range(nz):
        # lin_z[b]'s output gradient is the gradient at block b's input: the bias gradient of the layer writing it
        grads[f"lin_z.{b}.bias"] = grads[f"blocks.{b - 1}.fc_1.bias"] if b > 0 else grads["lin_in.bias"]
    return grads


def _lookup_point_grad(fused, entry, bwd, tables, latent, p, B, Gz, P):
    """d loss / d points through the latent lookup, (SB * B, 3), on HIP. From the forward's per-texel tables:
    sum_b Gz[b] . lin_z[b](interp(latent, p)) = sum_b Gz[b] . interp(table_b, p), the corner differences of the
    tables against each Gz row (ABI 15), no d_hidden x d_latent product per point for the feature gradient. Where
    that does not apply (or AVR_POINT_GRAD_VIA_FEATURES=1): the features' gradient through the lookup's adjoint."""
    dims = entry.dims
    H, nz = dims.d_hidden, dims.n_lin_z
    SB = p.shape[0]
    d_look = torch.empty(SB * B, 3, device=p.device, dtype=F32)
    if (not dims.spade and nz <= _lib.AVR_LOOKUP_GRAD_TERMS and tables.shape[0] == SB
            and os.environ.get("AVR_POINT_GRAD_VIA_FEATURES") != "1"):
        ld = Gz[0].stride(0)
        assert all(g.stride(0) == ld and g.stride(1) == 1 for g in Gz)
        gptr = [g.data_ptr() for g in Gz]
        for g0, n in scene_groups(SB):
            gr = (ctypes.c_void_p * nz)(*[g + g0 * B * ld * 4 for g in gptr])
            call("avr_latent_tables_grad_points", fused.views(range(g0, g0 + n)), n, ptr(tables[g0]),
                 tables.stride(0), tables.stride(1), nz, H, ptr(p[g0]), B, gr, ld, ptr(d_look[g0 * B]),
                 stream_of(d_look))
        return d_look
    g_feat = _feat_grad(fused, entry, bwd, Gz, P, SB * B)
    hwc = fused.latent_hwc_all(latent)
    for g0, n in scene_groups(SB):
        call("avr_latent_features_grad_points", fused.views(range(g0, g0 + n)), n, ptr(hwc[g0]), dims.d_latent,
             ptr(p[g0]), B, ptr(g_feat[g0 * B]), ptr(d_look[g0 * B]), stream_of(d_look))
    return d_look


def _point_grad_hip(fused, entry, bwd, tables, xyz, viewdirs, latent, p, G_in, Gz, P):
    """d loss / d xyz for the points alone (the adaptive renderer's band, fixed latent) on HIP: the lookup's part
    (_lookup_point_grad), then z_feature's added to it (ABI 16): d loss / d z_feature = G_in W_in (its
    positional-encoded columns only), then the encoding's and the rotation's adjoint per point in one launch.
    With stop_encoder_grad the looked-up latent is detached (models.py:810-811): z_feature's part alone.
    AVR_POINT_ZF_VIA_AUTOGRAD=1: torch autograd of z_features instead, the round-5 path, for A/B."""
    net, dims = fused.net, entry.dims
    SB, B, _ = xyz.shape
    d_look = None
    if not net.stop_encoder_grad:
        with torch.no_grad():
            d_look = _lookup_point_grad(fused, entry, bwd, tables, latent, p, B, Gz, P)
    if os.environ.get("AVR_POINT_ZF_VIA_AUTOGRAD") == "1":
        with torch.enable_grad():
            x = xyz.detach().requires_grad_(True)
            zft = net.z_features(x, viewdirs.detach())
            d_z, = torch.autograd.grad(zft, x, G_in @ P["lin_in.weight"].detach())
        return (d_z if d_look is None else d_look.reshape(SB, B, 3) + d_z).to(xyz.dtype)
    with torch.no_grad():
        d_zf = G_in @ P["lin_in.weight"].detach()[:, :3 + 6 * dims.num_freqs]
        if d_look is None:
            d_look = torch.empty(SB * B, 3, device=xyz.device, dtype=F32)
        for g0, n in scene_groups(SB):
            call("avr_zfeature_grad_points", fused.views(range(g0, g0 + n)), n, ptr(p[g0]), B, ptr(d_zf[g0 * B]),
                 d_zf.stride(0), dims.num_freqs, dims.freq_factor, int(not net.stop_encoder_grad),
                 ptr(d_look[g0 * B]), stream_of(d_look))
    return d_look.reshape(SB, B, 3).to(xyz.dtype)


class _FieldTrain(torch.autograd.Function):
    """Autograd of NewPixelNeRFNet.forward (models.py:739-863) for train.py's
    loss.backward() (train.py:108-114).

    forward: avr_field_fwd_points_train per scene (x3 MFMA, the inference
    kernel plus a store of every hidden GEMM input, its relu mask and the
    layer's running max) into one (layers, SB * B, d_hidden) buffer.
    backward: avr_field_bwd runs the input-gradient chain per scene (lin_out^T,
    then fc_1^T / fc_0^T per block with the relu masks, x3 MFMA) and writes the
    gradient at every layer output (_bwd_chain); avr_weight_grads then forms every
    weight and bias gradient in one batched split-K x3 GEMM over all samples
    (_weight_grads: fc_0 / fc_1 against the saved inputs, lin_z against the
    interpolated latent (grid_sample, models.py:266-273), lin_in against the
    positional-encoded input). The latent maps get the lookup's adjoint of
    sum_b G_z[b] W_z[b] on HIP when they require grad (latent_grad_hip:
    deterministic, no float atomics), the points their gradient on HIP as well
    (_point_grad_hip); what neither covers goes through torch's input functions
    (input_grads: one map shared by several scenes, AVR_LATENT_GRAD_VIA_AUTOGRAD=1)."""

    @staticmethod
    def forward(ctx, fused, coarse, names, xyz, viewdirs, latent, *params):
        SB, B, _ = xyz.shape
        entry = fused.packed(coarse)
        dims = entry.dims_as(_lib.FIELD_X3)
        H, nb = dims.d_hidden, dims.n_blocks
        n_l, Mt = 2 * nb + 1, SB * B
        dev = xyz.device
        out = torch.empty(SB, B, 4, device=dev, dtype=F32)
        act = torch.empty(n_l, Mt, H, device=dev, dtype=F32)
        act_max = torch.zeros(n_l + 1, device=dev, dtype=torch.int32)   # + max |z_feature|
        zs = dims.d_in + (-dims.d_in) % 4                                # z_feature rows padded to 16 B
        zf = torch.empty(Mt, zs, device=dev, dtype=F32)
        p = xyz.detach().to(F32).contiguous()
        v = viewdirs.reshape(SB, B, 3).detach().to(F32).contiguous()
        require_device(p, v)
        tables = fused.tables_batch(coarse, SB, fast=True, entry=entry)
        masks = []
        for g0, n in scene_groups(SB):     # one launch per group of scenes
            _, mask_n = size_query("avr_field_train_sizes", ctypes.byref(dims), n, B, n=2)
            views = fused.views(range(g0, g0 + n))
            mask = torch.empty(max(mask_n, 1), device=dev, dtype=torch.int32)
            call("avr_field_fwd_points_train", ctypes.byref(dims), views, n, ptr(entry.packed), ptr(tables[g0]),
                 ptr(p[g0]), ptr(v[g0]), B, ptr(out[g0]), ptr(act, g0 * B * H), Mt, ptr(mask), ptr(act_max),
                 ptr(zf, g0 * B * zs), zs, ptr(act_max, n_l), stream_of(p))
            masks.append((g0, n, mask))
        ctx.fused, ctx.coarse, ctx.names, ctx.entry = fused, coarse, names, entry
        ctx.act, ctx.act_max, ctx.masks, ctx.zf = act, act_max, masks, zf
        ctx.tables = tables
        ctx.save_for_backward(xyz, viewdirs, latent, out, *params)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        xyz, viewdirs, latent, out, *params = ctx.saved_tensors
        fused, entry, names = ctx.fused, ctx.entry, ctx.names
        net = fused.net
        P = dict(zip(names, params))
        dims = entry.dims_as(_lib.FIELD_X3)
        nb, nz = dims.n_blocks, dims.n_lin_z
        SB, B, _ = xyz.shape
        Mt = SB * B
        want_xyz = ctx.needs_input_grad[3]
        want_latent = ctx.needs_input_grad[5] and not net.stop_encoder_grad
        if B == 0:
            zeros = tuple(torch.zeros_like(p) if ctx.needs_input_grad[6 + i] else None for i, p in enumerate(params))
            return (None, None, None, torch.zeros_like(xyz) if want_xyz else None, None,
                    torch.zeros_like(latent) if want_latent else None) + zeros
        bwd = fused.packed_bwd(ctx.coarse, entry)
        grad_out = grad_out.to(F32).contiguous()
        act, act_max, zf = ctx.act, ctx.act_max, ctx.zf
        G, g_max = _bwd_chain(dims, entry, bwd, ctx.masks, B, Mt, out, grad_out, act)
        ctx.act = ctx.act_max = ctx.masks = ctx.zf = None
        # MLP inputs the lin_z / lin_in gradients contract against: the latent features (row-major) and z_feature
        # (the training forward stored it, padded to 16 B)
        p = xyz.detach().to(F32).contiguous()
        with torch.no_grad():
            lat_feat = lookup_features(fused, latent, p, SB, B)
        lat_max = fused.latent_max_bits(latent)   # |interpolated latent| <= max |latent| (convex blend)
        Gz = [G[2 * b - 1] if b > 0 else G[2 * nb] for b in range(nz)]
        # lin_out (4 outputs): d out through sigmoid / relu (torch: g * (1 - y) * y, g * (y > 0)), with its max
        d4, d4_max = ops.lin_out_act_bwd(grad_out, out)
        grads = _weight_grads(dims, Mt, G, g_max, act, act_max, lat_feat, lat_max, zf, d4, d4_max)
        d_latent = d_xyz = None
        points_on_hip = want_xyz and (net.stop_encoder_grad or (nz > 0 and SB <= latent.shape[0]))
        if points_on_hip and want_latent and latent_grad_on_hip(latent, SB):
            # both on HIP: the maps' gradient from the lookup's adjoint, the points' as when they alone want one
            fused.last_latent_grad = "hip"
            d_latent = latent_grad_hip(fused, latent, xyz, _feat_grad(fused, entry, bwd, Gz, P, Mt))
            d_xyz = _point_grad_hip(fused, entry, bwd, ctx.tables, xyz, viewdirs, latent, p, G[2 * nb], Gz, P)
        elif points_on_hip and not want_latent:
            d_xyz = _point_grad_hip(fused, entry, bwd, ctx.tables, xyz, viewdirs, latent, p, G[2 * nb], Gz, P)
        elif want_latent or want_xyz:
            g_feat = _feat_grad(fused, entry, bwd, Gz, P, Mt) if nz > 0 else None
            d_latent, d_xyz = train_common.mlp_input_grads(fused, xyz, viewdirs, latent, want_latent, want_xyz, g_feat,
                                                           G[2 * nb], P["lin_in.weight"])
        return train_common.backward_result(ctx.needs_input_grad, names, grads, d_xyz, d_latent)
