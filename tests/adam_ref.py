"""Float64 reference of the Adam step (avr_adam_step, include/avr.h) and the shared input of the Adam tests.

adam_ref restates the update rule in numpy float64 for prescribed gradients; test_cpu_adam.py checks it against
torch.optim.Adam on float64 CPU parameters. The GPU tests measure avr.optim.Adam and a default-constructed
torch.optim.Adam on the same device against its trajectory (within_bar)."""
import functools

import numpy as np
import torch

SETTINGS = {
    "defaults": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
    "weight_decay": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2),
    "other_betas": dict(lr=1e-2, betas=(0.5, 0.9), eps=1e-3, weight_decay=0.0),
}


def adam_ref(p0, grads, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, m0=None, v0=None, step0=0):
    """The trajectory [(p, m, v) after step 1, 2, ...] of one array from p0 (and m0, v0 = 0, step0 steps taken)
    under the gradients `grads` (one array per step), everything in float64:
        g = grad + weight_decay * p;  m += (g - m) (1 - beta1);  v = v beta2 + (1 - beta2) g g;  t = step + 1
        p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)"""
    b1, b2 = betas
    p = np.asarray(p0, np.float64).copy()
    m = np.zeros_like(p) if m0 is None else np.asarray(m0, np.float64).copy()
    v = np.zeros_like(p) if v0 is None else np.asarray(v0, np.float64).copy()
    out = []
    with np.errstate(all="ignore"):
        for k, g in enumerate(grads):
            g = np.asarray(g, np.float64)
            if weight_decay != 0:
                g = g + weight_decay * p
            m = m + (g - m) * (1 - b1)
            v = v * b2 + (1 - b2) * g * g
            t = step0 + k + 1
            p = p - (lr / (1 - b1 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
            out.append((p.copy(), m.copy(), v.copy()))
    return out


def case_specs(chunk):
    """(name, shape, kind) of the shared input's tensors; chunk = AVR_ADAM_CHUNK. Kinds: plain; param_view (the
    parameter starts one float into a larger buffer: 4-B aligned only); grad_view (its .grad does); transposed (a
    dense parameter that is not contiguous); no_grad (.grad stays None); empty (numel 0)."""
    C = chunk
    specs = [(f"n{n}", (n,), "plain") for n in (1, 3, 4, 5, 255, 256, 257, C - 1, C, C + 1, 2 * C + 5)]
    specs += [("w4x64", (4, 64), "plain"), ("w64x42", (64, 42), "plain"), ("w64x64", (64, 64), "plain"),
              ("w42x64_t", (64, 42), "transposed"),
              ("param_view", (C + 7,), "param_view"), ("grad_view", (2 * C + 2,), "grad_view"),
              ("no_grad", (37,), "no_grad"), ("empty", (0,), "empty")]
    return specs


def init_values(specs, seed=0):
    """fp32 start values 0.1 N(0, 1) per spec."""
    rng = np.random.default_rng(seed)
    return [(0.1 * rng.standard_normal(shape)).astype(np.float32) for _, shape, _ in specs]


def step_grads(specs, n_steps, seed=1):
    """Per step, per spec: fp32 gradients N(0, 1) 10^k with k drawn per element from the integers [-8, 3), every
    17th element exactly 0."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_steps):
        gs = []
        for _, shape, _ in specs:
            g = rng.standard_normal(shape) * 10.0 ** rng.integers(-8, 3, size=shape)
            g.reshape(-1)[::17] = 0.0
            gs.append(g.astype(np.float32))
        out.append(gs)
    return out


def make_params(specs, values, device, dtype=torch.float32, plain=False):
    """Parameters of the shared input on `device` (plain: every one an ordinary contiguous tensor, what the torch
    twin steps) and, per parameter, the .grad tensor to fill in place (None for no_grad). Gradients are zero."""
    params, grads = [], []
    for (name, shape, kind), val in zip(specs, values):
        t = torch.from_numpy(val).to(device=device, dtype=dtype)
        n = t.numel()
        if kind == "param_view" and not plain:
            buf = torch.zeros(n + 8, device=device, dtype=dtype)
            buf[1:n + 1] = t
            p = torch.nn.Parameter(buf[1:n + 1])
            assert p.data_ptr() % 16 == 4
        elif kind == "transposed" and not plain:
            buf = torch.zeros(shape[1], shape[0], device=device, dtype=dtype)
            buf.t().copy_(t)
            p = torch.nn.Parameter(buf.t())
            assert not p.is_contiguous()
        else:
            p = torch.nn.Parameter(t.clone())
        if kind == "no_grad":
            g = None
        elif kind == "grad_view" and not plain:
            g = torch.zeros(n + 8, device=device, dtype=dtype)[1:n + 1]
            assert g.data_ptr() % 16 == 4
        else:
            g = torch.zeros_like(p, memory_format=torch.preserve_format)
        p.grad = g
        params.append(p)
        grads.append(g)
    return params, grads


def fill_grads(grads, values):
    """Copy one step's gradient values into the .grad tensors in place (their addresses stay)."""
    for g, val in zip(grads, values):
        if g is not None:
            g.copy_(torch.from_numpy(val).to(device=g.device, dtype=g.dtype))


@functools.lru_cache(maxsize=None)
def case_trajectory(chunk, setting, n_steps):
    """The shared input and its float64 trajectory under SETTINGS[setting], computed once per process:
    (specs, init values, per-step gradients, per-spec trajectories [(p, m, v)] or None for no_grad). Read-only."""
    specs = case_specs(chunk)
    values = init_values(specs)
    grads = step_grads(specs, n_steps)
    traj = [None if kind == "no_grad" else adam_ref(values[i], [g[i] for g in grads], **SETTINGS[setting])
            for i, (_, _, kind) in enumerate(specs)]
    return specs, values, grads, traj


def errors(got, ref):
    """max |got - ref| of one array against the float64 one (0 for an empty array)."""
    got = np.asarray(got, np.float64)
    return float(np.abs(got - ref).max()) if got.size else 0.0


def within_bar(what, hip, tor, ref):
    """The project's fp32-equivalence bar (tests/test_gpu_train.py _compare64) on one array: against the float64
    reference, avr's max abs error is within twice torch's own plus the rounding of one fp32 store of the
    array's largest value. Returns (err_hip, err_torch, floor)."""
    ref = np.asarray(ref, np.float64)
    eh, et = errors(hip, ref), errors(tor, ref)
    floor = 2.0 ** -24 * (float(np.abs(ref).max()) if ref.size else 0.0)
    print(f"{what}: err_hip {eh:.3e} err_torch {et:.3e} floor {floor:.3e}")
    assert eh <= 2.0 * et + floor, f"{what}: avr err {eh:.3e} vs torch err {et:.3e}, floor {floor:.3e}"
    return eh, et, floor
