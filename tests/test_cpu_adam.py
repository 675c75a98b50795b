"""CPU-only checks of avr.optim.Adam / avr_adam_step (ABI 18): the C entry's argument checks run before any HIP
call, the float64 reference of the GPU tests (tests/adam_ref.py) agrees with torch.optim.Adam on float64 CPU
parameters, the constructor takes train.py:299's call and refuses what the kernel does not implement, and the
argument checks pass a host AddressSanitizer build driven by a stand-alone program. No kernel is launched."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from adam_ref import adam_ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "adaptive-volume-rendering_amd")
D = ctypes.c_double


def test_library_is_abi_18_and_exports_adam_step():
    from avr import _lib
    lib = _lib.load()
    assert lib.avr_version() == 18 == _lib.ABI_VERSION
    assert "avr_adam_step" in _lib.EXPORTED and hasattr(lib, "avr_adam_step")
    header = open(os.path.join(REPO, "include", "avr.h")).read()
    assert int(re.search(r"#define AVR_ADAM_CHUNK (\d+)", header).group(1)) == _lib.ADAM_CHUNK
    assert int(re.search(r"#define AVR_ADAM_MAX_TENSORS (\d+)", header).group(1)) == _lib.ADAM_MAX_TENSORS
    assert ctypes.sizeof(_lib.AdamTensor) == 40      # five 8-byte fields: ops.adam_step fills it as int64s


def test_adam_step_argument_checks():
    """Every refusal of include/avr.h, through ctypes with null or host-only arguments: code 1001 and the stated
    message; zero tensors is a no-op that leaves the counter alone."""
    from avr import _lib
    lib = _lib.load()
    f = lib.avr_adam_step
    host = (ctypes.c_float * 8)()
    hp = ctypes.addressof(host)
    step = ctypes.c_float(3.0)
    sp = ctypes.addressof(step)
    ok = (D(1e-3), D(0.9), D(0.999), D(1e-8), D(0.0))

    def arr(*entries):
        return (_lib.AdamTensor * len(entries))(*[_lib.AdamTensor(*e) for e in entries])

    good = (hp, hp, hp, hp, 8)
    err = lambda: lib.avr_last_error_string()  # noqa: E731
    assert f(None, 0, *ok, None, None) == 0
    assert f(arr(good), 0, *ok, sp, None) == 0
    assert f(arr(good), -1, *ok, sp, None) == 1001 and b"n_tensors" in err()
    assert f(None, 1, *ok, sp, None) == 1001 and b"null" in err()
    assert f(arr(good), 1, *ok, None, None) == 1001 and b"null" in err()
    assert f(arr(good, (hp, hp, hp, hp, -1)), 2, *ok, sp, None) == 1001 and b"numel" in err()
    for slot in range(4):
        bad = list(good)
        bad[slot] = None
        assert f(arr(good, (None, None, None, None, 0), tuple(bad)), 3, *ok, sp, None) == 1001
        assert b"null" in err() and b"tensor 2" in err()
    for k, (value, name) in enumerate([(-1e-3, b"lr"), (1.0, b"beta1"), (1.0, b"beta2"), (-1e-8, b"eps"),
                                       (-1e-2, b"weight_decay")]):
        hyper = list(ok)
        hyper[k] = D(value)
        assert f(arr(good), 1, *hyper, sp, None) == 1001 and name in err(), name
    for k, name in ((1, b"beta1"), (2, b"beta2")):
        hyper = list(ok)
        hyper[k] = D(-0.25)
        assert f(arr(good), 1, *hyper, sp, None) == 1001 and name in err()
    assert f(arr(good), 1, D(float("nan")), *ok[1:], sp, None) == 1001 and b"lr" in err()
    assert step.value == 3.0 and not any(host)


@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_adam_ref_agrees_with_torch_float64(weight_decay):
    """adam_ref against torch.optim.Adam on float64 CPU parameters over 25 steps: within 1e-12 of max |p| (the two
    differ by rounding order only, about 1e-16 at |p| ~ 0.4)."""
    rng = np.random.default_rng(5)
    p0 = 0.1 * rng.standard_normal(4000)
    grads = [rng.standard_normal(4000) * 10.0 ** rng.integers(-8, 3, size=4000) for _ in range(25)]
    traj = adam_ref(p0, grads, weight_decay=weight_decay)
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([p], weight_decay=weight_decay)
    for k, g in enumerate(grads):
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        rp, rm, rv = traj[k]
        st = opt.state[p]
        scale = float(np.abs(rp).max())
        assert float(np.abs(p.detach().numpy() - rp).max()) <= 1e-12 * scale, k
        assert float(np.abs(st["exp_avg"].numpy() - rm).max()) <= 1e-12 * float(np.abs(rm).max()), k
        assert float(np.abs(st["exp_avg_sq"].numpy() - rv).max()) <= 1e-12 * float(np.abs(rv).max()), k
    assert float(opt.state[p]["step"]) == 25


def test_adam_ref_continues_from_a_state():
    rng = np.random.default_rng(6)
    p0, grads = rng.standard_normal(50), [rng.standard_normal(50) for _ in range(5)]
    whole = adam_ref(p0, grads, weight_decay=1e-2)
    p, m, v = whole[2]
    rest = adam_ref(p, grads[3:], weight_decay=1e-2, m0=m, v0=v, step0=3)
    for a, b in zip(rest[-1], whole[-1]):
        assert np.array_equal(a, b)


def test_constructor_accepts_train_py_call_and_refuses_the_rest():
    import avr
    from avr.optim import Adam
    assert avr.Adam is Adam and issubclass(Adam, torch.optim.Optimizer)
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
    opt = Adam(lr=5e-4, params=ps)                                   # train.py:299
    assert opt.param_groups[0]["lr"] == 5e-4
    Adam(ps, lr=1e-4, capturable=True, fused=True)                   # call sites written for the capturable form
    Adam(ps, foreach=True)
    assert set(opt.state_dict()["param_groups"][0]) == set(torch.optim.Adam(ps).state_dict()["param_groups"][0])
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(differentiable=True), dict(lr=torch.tensor(1e-3))):
        with pytest.raises(ValueError):
            Adam(ps, **kw)
    for kw, msg in ((dict(lr=-1.0), "Invalid learning rate: -1.0"), (dict(eps=-1.0), "Invalid epsilon value: -1.0"),
                    (dict(betas=(1.0, 0.9)), "Invalid beta parameter at index 0: 1.0"),
                    (dict(betas=(0.9, -0.1)), "Invalid beta parameter at index 1: -0.1"),
                    (dict(weight_decay=-1.0), "Invalid weight_decay value: -1.0")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            Adam(ps, **kw)
        with pytest.raises(ValueError, match=re.escape(msg)):      # torch's wording
            torch.optim.Adam(ps, **kw)


def test_step_on_cpu_parameters_raises():
    from avr._lib import AVRError
    from avr.optim import Adam
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.ones(4))]
    opt = Adam(ps)
    opt.step()                       # no gradient anywhere: nothing to do, no state
    assert len(opt.state) == 0
    ps[1].grad = torch.ones(4)
    with pytest.raises(AVRError, match="parameter 1 .*no CPU path"):
        opt.step()
    assert len(opt.state[ps[1]]) == 0 and bool((ps[1] == 1).all())
    # a hyper-parameter made invalid after construction is refused at the step that would use it
    opt.param_groups[0]["lr"] = -1.0
    with pytest.raises(ValueError, match="Invalid learning rate"):
        opt.step()


def test_load_state_dict_refuses_mixed_step_counts():
    """Host-only: a torch.optim.Adam state (CPU `step` tensors) loads; one whose parameters disagree on the step
    count inside a group raises ValueError."""
    from avr.optim import Adam
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.ones(4))]
    ref = torch.optim.Adam(ps, lr=1e-2)
    for p in ps:
        p.grad = torch.ones_like(p)
    ref.step()
    ref.step()
    sd = ref.state_dict()
    opt = Adam(ps, lr=1e-2)
    opt.load_state_dict(sd)
    steps = [opt.state[p]["step"] for p in ps]
    assert steps[0] is steps[1] and float(steps[0]) == 2 and steps[0].dtype == torch.float32
    back = opt.state_dict()["state"]
    assert back[0]["step"] is not back[1]["step"] and set(back[0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert torch.equal(back[1]["exp_avg"], sd["state"][1]["exp_avg"])
    sd["state"][1]["step"] = torch.tensor(5.0)
    fresh = Adam(ps, lr=1e-2)
    with pytest.raises(ValueError, match="different step counts"):
        fresh.load_state_dict(sd)
    assert len(fresh.state) == 0                 # refused before anything was replaced


def test_adam_abi_check_under_host_asan():
    """tests/adam_abi_check.c against the host-AddressSanitizer build of the library (`make asan-adam`), run as a
    program of its own: nothing is preloaded and nothing is loaded into Python."""
    b = subprocess.run(["make", "-C", PKG, "asan-adam", "-j8"], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([os.path.join(PKG, "build", "adam_abi_check_asan")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "adam_abi_check: 0 failure(s)" in r.stdout
    assert "AddressSanitizer" not in r.stderr


def test_load_state_dict_gives_the_moments_the_parameters_strides():
    """A state saved over contiguous parameters, loaded over a dense parameter with other strides (a transposed
    view): exp_avg and exp_avg_sq take the parameter's strides and keep their values element for element (the
    kernel walks the four arrays in one memory order)."""
    from avr.optim import Adam
    src = torch.nn.Parameter(torch.zeros(3, 5))
    ref = torch.optim.Adam([src])
    src.grad = torch.arange(15.0).reshape(3, 5)
    ref.step()
    dst = torch.nn.Parameter(torch.zeros(5, 3).t())
    opt = Adam([dst])
    opt.load_state_dict(ref.state_dict())
    for key in ("exp_avg", "exp_avg_sq"):
        assert opt.state[dst][key].stride() == dst.stride() == (1, 3)
        assert torch.equal(opt.state[dst][key], ref.state[src][key])
