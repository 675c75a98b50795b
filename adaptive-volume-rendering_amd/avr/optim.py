"""avr.optim.Adam: train.py's optimizer (train.py:299, stepped at :112-114) as one HIP launch sequence.

    from avr.optim import Adam        # instead of torch.optim.Adam; the constructor call stays as it is
"""
import torch
from torch.optim import Optimizer

from . import ops
from ._lib import AVRError

F32 = torch.float32
_REFUSED = ("amsgrad", "maximize", "differentiable", "decoupled_weight_decay")


def _check_hyper(lr, betas, eps, weight_decay):
    if isinstance(lr, torch.Tensor):
        raise ValueError("avr.optim.Adam takes a float lr: a tensor lr is not supported (the launch takes the "
                         "learning rate by value; set group['lr'] from the host schedule)")
    if not 0.0 <= lr:
        raise ValueError(f"Invalid learning rate: {lr}")
    if not 0.0 <= eps:
        raise ValueError(f"Invalid epsilon value: {eps}")
    for i in (0, 1):
        if isinstance(betas[i], torch.Tensor):
            raise ValueError(f"avr.optim.Adam takes float betas: betas[{i}] is a tensor")
        if not 0.0 <= betas[i] < 1.0:
            raise ValueError(f"Invalid beta parameter at index {i}: {betas[i]}")
    if not 0.0 <= weight_decay:
        raise ValueError(f"Invalid weight_decay value: {weight_decay}")


class Adam(Optimizer):
    """torch.optim.Adam's update of fp32 parameters on a HIP device by csrc/adam.hip (avr_adam_step): per param
    group one multi-tensor launch per 88 parameters plus a one-wave launch that advances the step counter,
    whatever the number of parameters; no torch kernel, no host read, no allocation after the first step.

    The constructor takes torch.optim.Adam's arguments, so `Adam(lr=opt.lr, params=...)` and call sites written
    for `torch.optim.Adam(..., capturable=True, fused=True)` stay as they are. foreach, capturable and fused are
    accepted and ignored: the step is always one fused kernel and always capturable (the step count is one fp32
    scalar in device memory per param group that only the kernel reads, and every parameter's state['step'] of
    the group is that tensor). amsgrad, maximize, differentiable, decoupled_weight_decay, a tensor lr and invalid
    hyper-parameters raise ValueError.

    The hyper-parameters are read from the param group at every step(), so a host-side learning-rate schedule
    works in eager steps. A HIP-graph capture of step() (torch.cuda.graph, avr.graphs.GraphedTrainStep) bakes in
    their values of capture time, as torch's capturable Adam does with a float lr: capture again after changing
    them. Take one eager step before capturing (the first step allocates the state).

    Like torch's fused Adam, the kernel writes the parameters without advancing their version counters. An eager
    step() advances avr.field.param_generation() through torch's optimizer-step hook, so FusedField's packed
    weights and tables are rebuilt after it; a graph replay runs no host hook: call
    avr.field.bump_param_generation() after a replay that steps (GraphedTrainStep does).

    Parameters whose .grad is None are skipped and get no state. A parameter that first gets a gradient after
    others of its group have stepped joins the group's step count (torch would start its own count at 1).
    state_dict() has torch.optim.Adam's layout (per parameter `step`, a 0-dim fp32 tensor of its own, `exp_avg`,
    `exp_avg_sq`; the same param_groups keys) and loads into torch.optim.Adam; load_state_dict() takes a
    torch.optim.Adam state (its `step` may be a CPU tensor) and raises ValueError where the parameters of one
    group carry different step counts.

    step() raises for what the kernel does not cover, naming the parameter's index in its group: a parameter not
    on a HIP device (AVRError: there is no CPU path), a dtype other than fp32, a sparse gradient, a parameter that
    is not dense and non-overlapping, a gradient whose strides differ from its parameter's, and parameters on
    more than one device.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        _check_hyper(lr, betas, eps, weight_decay)
        defaults = {"lr": lr, "betas": (betas[0], betas[1]), "eps": eps, "weight_decay": weight_decay,
                    "amsgrad": amsgrad, "maximize": maximize, "foreach": foreach, "capturable": capturable,
                    "differentiable": differentiable, "fused": fused,
                    "decoupled_weight_decay": decoupled_weight_decay}
        for name in _REFUSED:
            if defaults[name]:
                raise ValueError(f"avr.optim.Adam does not implement {name}=True")
        super().__init__(params, defaults)

    @staticmethod
    def _refuse(gi, i, p, g, dev):
        """Why parameter i of group gi cannot be stepped (the slow half of step()'s check)."""
        who = f"avr.optim.Adam: parameter {i} of group {gi}"
        if g.is_sparse or g.layout != torch.strided or p.layout != torch.strided:
            raise ValueError(f"{who} has a sparse gradient or layout ({p.layout}, grad {g.layout}); only dense "
                             "tensors are supported")
        if not p.is_cuda or not g.is_cuda:
            raise AVRError(f"{who} is on {p.device} (grad on {g.device}): the step runs on a ROCm/HIP device, "
                           "there is no CPU path")
        if p.dtype != F32 or g.dtype != F32:
            raise ValueError(f"{who} is {p.dtype} (grad {g.dtype}): only float32 parameters are supported")
        if p.device != dev or g.device != dev:
            raise ValueError(f"{who} is on {p.device} (grad on {g.device}), others on {dev}: the "
                             "parameters of one optimizer must be on one device")
        if not torch.ops.aten.is_non_overlapping_and_dense(p):
            raise ValueError(f"{who} is not dense and non-overlapping (shape {tuple(p.shape)}, strides {p.stride()})")
        if g.stride() != p.stride() or g.shape != p.shape:
            raise ValueError(f"{who}: the gradient's strides {g.stride()} differ from the parameter's {p.stride()}")
        raise ValueError(f"{who} cannot be stepped by the HIP kernel")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        dev = None   # of the first parameter that has a gradient: every other one must be there too
        for gi, group in enumerate(self.param_groups):
            for name in _REFUSED:
                if group.get(name):
                    raise ValueError(f"avr.optim.Adam does not implement {name}=True (param group {gi})")
            _check_hyper(group["lr"], group["betas"], group["eps"], group["weight_decay"])
            found, counter, fresh = [], None, False
            for i, p in enumerate(group["params"]):
                g = p.grad
                if g is None:
                    continue
                if dev is None:
                    dev = p.device
                # what the kernel needs, in one expression; _refuse says which part failed
                if not (p.dtype is F32 and g.dtype is F32 and p.is_cuda and g.layout is torch.strided
                        and p.device == dev and g.device == dev and g.stride() == p.stride()
                        and g.shape == p.shape
                        and (p.is_contiguous() or torch.ops.aten.is_non_overlapping_and_dense(p))):
                    self._refuse(gi, i, p, g, dev)
                state = self.state[p]
                if len(state) == 0:
                    fresh = True
                elif counter is None:
                    counter = state["step"]
                found.append((p, g, state))
            if not found:
                continue
            if fresh:   # after every parameter of the group passed: a refused step leaves no half-made state
                if counter is None:
                    counter = torch.zeros((), dtype=F32, device=dev)
                for p, g, state in found:
                    if len(state) == 0:
                        state["step"] = counter
                        state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                        state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            tensors = [(p, g, state["exp_avg"], state["exp_avg_sq"]) for p, g, state in found]
            beta1, beta2 = group["betas"]
            ops.adam_step(tensors, group["lr"], beta1, beta2, group["eps"], group["weight_decay"], counter)
        return loss

    def state_dict(self):
        """torch.optim.Adam's layout; every parameter gets a `step` tensor of its own (a copy of its group's
        counter), so the state loads into an optimizer that advances each parameter's count by itself."""
        sd = super().state_dict()
        sd["state"] = {k: {**v, "step": v["step"].clone()} if "step" in v else dict(v) for k, v in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """Takes this class's state or torch.optim.Adam's (`step` on the CPU or the device, a tensor or a number).
        The parameters of one group must agree on the step count: the group continues with one device counter."""
        saved = state_dict["state"]
        for gi, group in enumerate(state_dict["param_groups"]):   # refused before anything is replaced
            counts = {float(saved[k]["step"]) for k in group["params"] if "step" in saved.get(k, ())}
            if len(counts) > 1:
                raise ValueError(f"avr.optim.Adam: the parameters of group {gi} carry different step counts "
                                 f"{sorted(counts)}; one group keeps one counter")
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            held = [(p, self.state[p]) for p in group["params"] if len(self.state.get(p, ())) != 0]
            if not held:
                continue
            for p, s in held:   # the kernel walks p, m and v in one element order: the moments take p's strides
                for key in ("exp_avg", "exp_avg_sq"):
                    if s[key].stride() != p.stride():
                        s[key] = torch.empty_like(p, memory_format=torch.preserve_format).copy_(s[key])
            counter = torch.full((), float(held[0][1]["step"]), dtype=F32, device=held[0][1]["exp_avg"].device)
            for _, s in held:
                s["step"] = counter
