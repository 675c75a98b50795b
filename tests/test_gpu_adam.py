"""avr.optim.Adam (csrc/adam.hip, ABI 18) on the device against the float64 trajectory of tests/adam_ref.py.

The bar is the project's fp32-equivalence bar (tests/test_gpu_train.py _compare64) on each of the optimizer's three
arrays -- param, exp_avg, exp_avg_sq, each over all of the optimizer's elements: err_hip <= 2 err_torch +
2^-24 max |array|, both errors max abs differences from the float64 trajectory, err_torch that of a
default-constructed torch.optim.Adam on clones on the same device. It is not applied to one small tensor by itself:
torch's foreach kernels round in another order than the rule of include/avr.h (alpha * (g * g) with a * b + c
contracted; this library is built with -ffp-contract=off), so on a handful of elements twice torch's error is a
draw of its rounding luck, not an error scale. Where a test has to show that every single tensor was updated
correctly (the long list), each element is held to a bound that follows from the fp32 format alone
(_one_step_format_bound)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from adam_ref import (SETTINGS, adam_ref, case_trajectory, fill_grads, make_params, within_bar)  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def _chunk():
    from avr import _lib
    return _lib.ADAM_CHUNK


def _np(t):
    return t.detach().cpu().numpy()


def _state(opt, p):
    return opt.state[p] if p in opt.state else {}


def _triples(opt, params):
    """Per parameter (p, exp_avg, exp_avg_sq) as numpy in logical element order, None without state."""
    out = []
    for p in params:
        st = _state(opt, p)
        out.append((_np(p), _np(st["exp_avg"]), _np(st["exp_avg_sq"])) if len(st) else None)
    return out


def _check(tag, hip, tor, ref):
    """The bar on avr's (hip) and torch's (tor) triples against the reference triples of one step."""
    live = [i for i, r in enumerate(ref) if r is not None]
    for q, qn in enumerate(("param", "exp_avg", "exp_avg_sq")):
        cat = lambda rows: np.concatenate([np.asarray(rows[i][q]).reshape(-1) for i in live])  # noqa: E731
        within_bar(f"{tag} {qn}", cat(hip), cat(tor), cat(ref))


def _one_step_format_bound(name, got, ref, lr):
    """After ONE step from zero state without weight decay, every element against float64, from the roundings of
    the rule alone (d = 2^-24, the relative error of one fp32 rounding; 1 - beta and the bias factors are rounded
    once to fp32 too): m = (g - 0) * w1: 2 roundings, 2 d |m|; v = (w2 * g) * g: 3 roundings, 3 d |v|;
    p = p + s * (m / (sqrt(v) / c + eps)): the update is at most lr in size and carries the roundings of s, m,
    sqrt(v) (half of v's), the sqrt, c, two divisions, an addition and a product, under 10 d lr, and the final
    addition d |p|. Held with a 1.25 margin for the second-order terms: 2.5 d |m|, 3.75 d |v|, 1.25 d (|p| + 10 lr)."""
    d = 2.0 ** -24
    p, m, v = (np.asarray(a, np.float64) for a in got)
    rp, rm, rv = ref
    assert (np.abs(m - rm) <= 2.5 * d * np.abs(rm)).all(), (name, "exp_avg")
    assert (np.abs(v - rv) <= 3.75 * d * np.abs(rv)).all(), (name, "exp_avg_sq")
    assert (np.abs(p - rp) <= 1.25 * d * (np.abs(rp) + 10 * lr)).all(), (name, "param")


def _twins(specs, values, setting, avr_cls=None):
    from avr.optim import Adam
    ph, gh = make_params(specs, values, DEV)
    pt, gt = make_params(specs, values, DEV, plain=True)
    return (ph, gh, (avr_cls or Adam)(ph, **SETTINGS[setting])), (pt, gt, torch.optim.Adam(pt, **SETTINGS[setting]))


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_one_step_and_25_steps_within_the_bar(setting):
    specs, values, grads, traj = case_trajectory(_chunk(), setting, 25)
    (ph, gh, oh), (pt, gt, ot) = _twins(specs, values, setting)
    for k in range(25):
        fill_grads(gh, grads[k])
        fill_grads(gt, grads[k])
        oh.step()
        ot.step()
        if k in (0, 24):
            ref = [None if t is None else t[k] for t in traj]
            _check(f"{setting} step {k + 1}", _triples(oh, ph), _triples(ot, pt), ref)
    kinds = [kind for _, _, kind in specs]
    i = kinds.index("no_grad")
    assert np.array_equal(_np(ph[i]), values[i]) and len(_state(oh, ph[i])) == 0
    e = kinds.index("empty")
    assert ph[e].numel() == 0 and float(_state(oh, ph[e])["step"]) == 25
    steps = {id(_state(oh, p)["step"]) for p in ph if len(_state(oh, p))}
    assert len(steps) == 1                       # one device counter per param group


def test_list_longer_than_one_launch():
    """More tensors than one launch's argument block holds (ADAM_MAX_TENSORS + 3, numel 1..7): the optimizer's
    arrays are within the bar, every element of every tensor within the fp32 format's bound of one step, and the
    counter advanced by exactly 1."""
    from avr import _lib
    from avr.optim import Adam
    n = _lib.ADAM_MAX_TENSORS + 3
    specs = [(f"t{i}", (1 + i % 7,), "plain") for i in range(n)]
    rng = np.random.default_rng(3)
    values = [(0.1 * rng.standard_normal(s)).astype(np.float32) for _, s, _ in specs]
    grads = [rng.standard_normal(s).astype(np.float32) for _, s, _ in specs]
    ph, gh = make_params(specs, values, DEV)
    pt, gt = make_params(specs, values, DEV, plain=True)
    oh, ot = Adam(ph), torch.optim.Adam(pt)
    fill_grads(gh, grads)
    fill_grads(gt, grads)
    oh.step()
    ot.step()
    ref = [adam_ref(values[i], [grads[i]])[0] for i in range(n)]
    th = _triples(oh, ph)
    _check("long list", th, _triples(ot, pt), ref)
    for i in range(n):
        assert not np.array_equal(th[i][0], values[i]), i
        _one_step_format_bound(specs[i][0], th[i], ref[i], 1e-3)
    assert float(oh.state[ph[0]]["step"]) == 1.0 and oh.state[ph[-1]]["step"] is oh.state[ph[0]]["step"]


def test_non_finite_gradients_propagate_as_in_torch():
    """One NaN and one +inf in a gradient, at a 16-B-path element and at a tail element (and the other way
    round): isnan of p, m, v equals torch's elementwise, also after a further finite step; every other element is
    within the bar."""
    from avr.optim import Adam
    C = _chunk()
    specs = [("a", (C + 3,), "plain"), ("b", (C + 3,), "plain")]
    rng = np.random.default_rng(8)
    values = [(0.1 * rng.standard_normal(s)).astype(np.float32) for _, s, _ in specs]
    grads = [[rng.standard_normal(s).astype(np.float32) for _, s, _ in specs] for _ in range(2)]
    grads[0][0][5], grads[0][0][C + 1] = np.nan, np.inf
    grads[0][1][9], grads[0][1][C + 2] = np.inf, np.nan
    ph, gh = make_params(specs, values, DEV)
    pt, gt = make_params(specs, values, DEV, plain=True)
    oh, ot = Adam(ph), torch.optim.Adam(pt)
    traj = [adam_ref(values[i], [g[i] for g in grads]) for i in range(2)]
    for k in range(2):
        fill_grads(gh, grads[k])
        fill_grads(gt, grads[k])
        oh.step()
        ot.step()
        th, tt = _triples(oh, ph), _triples(ot, pt)
        for i in range(2):
            touched = np.zeros(C + 3, bool)
            for q in range(3):
                assert np.array_equal(np.isnan(th[i][q]), np.isnan(tt[i][q])), (k, i, q)
                touched |= ~np.isfinite(tt[i][q]) | ~np.isfinite(traj[i][k][q])
            assert touched.sum() == 2 and np.isnan(th[i][0]).sum() == 2     # p: NaN at both, nowhere else
            for q, qn in enumerate(("param", "exp_avg", "exp_avg_sq")):
                within_bar(f"non-finite step {k + 1} {specs[i][0]} {qn}", th[i][q][~touched], tt[i][q][~touched],
                           traj[i][k][q][~touched])


def test_two_runs_are_bit_identical():
    specs, values, grads, _ = case_trajectory(_chunk(), "defaults", 25)
    from avr.optim import Adam
    runs = []
    for _ in range(2):
        ph, gh = make_params(specs, values, DEV)
        opt = Adam(ph)
        for k in range(5):
            fill_grads(gh, grads[k])
            opt.step()
        runs.append((ph, opt))
    (pa, oa), (pb, ob) = runs
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        for key in ("exp_avg", "exp_avg_sq"):
            if len(_state(oa, a)):
                assert torch.equal(oa.state[a][key], ob.state[b][key])


def test_captured_step_equals_eager_steps():
    """One eager warm-up step, opt.step() captured into a single-stream graph, the static .grad tensors refilled in
    place and 3 replays: p, m, v equal a twin's 4 eager steps bit for bit, and state['step'] reads 4."""
    from avr.optim import Adam
    specs, values, grads, _ = case_trajectory(_chunk(), "defaults", 25)
    ph, gh = make_params(specs, values, DEV)
    pe, ge = make_params(specs, values, DEV)
    oh, oe = Adam(ph), Adam(pe)
    for k in range(4):
        fill_grads(ge, grads[k])
        oe.step()
    fill_grads(gh, grads[0])
    oh.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        oh.step()
    torch.cuda.current_stream().wait_stream(side)
    for k in range(1, 4):
        fill_grads(gh, grads[k])
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(ph, pe):
        assert torch.equal(a, b)
        if len(_state(oe, b)):
            assert torch.equal(oh.state[a]["exp_avg"], oe.state[b]["exp_avg"])
            assert torch.equal(oh.state[a]["exp_avg_sq"], oe.state[b]["exp_avg_sq"])
            assert float(oh.state[a]["step"]) == 4.0 == float(oe.state[b]["step"])


def test_checkpoints_interchange_with_torch_adam():
    """3 steps here, the state loaded into torch.optim.Adam over clones, 2 more steps in each: within the bar; the
    same from a torch state with CPU `step` tensors into avr.optim.Adam; a state whose steps differ inside a group
    is refused."""
    from avr.optim import Adam
    specs, values, grads, traj = case_trajectory(_chunk(), "defaults", 25)
    ref = [None if t is None else t[4] for t in traj]

    def clone_values(params):
        return [_np(p).copy() for p in params]

    for first in ("avr", "torch"):
        if first == "avr":
            pa, ga = make_params(specs, values, DEV)
            oa = Adam(pa)
        else:
            pa, ga = make_params(specs, values, DEV, plain=True)
            oa = torch.optim.Adam(pa)
        for k in range(3):
            fill_grads(ga, grads[k])
            oa.step()
        sd = copy.deepcopy(oa.state_dict())
        live = [i for i, t in enumerate(traj) if t is not None]
        assert sorted(sd["state"]) == live
        assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} and s["step"].dtype == torch.float32
                   and s["step"].dim() == 0 and float(s["step"]) == 3 for s in sd["state"].values())
        if first == "torch":
            assert all(s["step"].device.type == "cpu" for s in sd["state"].values())
        pb, gb = make_params(specs, clone_values(pa), DEV, plain=(first == "avr"))
        ob = torch.optim.Adam(pb) if first == "avr" else Adam(pb)
        ob.load_state_dict(sd)
        for k in range(3, 5):
            for g_, o_ in ((ga, oa), (gb, ob)):
                fill_grads(g_, grads[k])
                o_.step()
        ta, tb = _triples(oa, pa), _triples(ob, pb)
        hip, tor = (ta, tb) if first == "avr" else (tb, ta)
        _check(f"interchange from {first}", hip, tor, ref)
        assert all(float(_state(ob, p)["step"]) == 5 for p in pb if len(_state(ob, p)))
    bad = copy.deepcopy(sd)
    bad["state"][live[1]]["step"] = torch.tensor(7.0)
    with pytest.raises(ValueError, match="different step counts"):
        Adam(make_params(specs, values, DEV)[0]).load_state_dict(bad)


def test_step_refuses_what_the_kernel_does_not_cover():
    from avr.optim import Adam
    good = torch.nn.Parameter(torch.zeros(8, device=DEV))
    good.grad = torch.ones(8, device=DEV)

    def refused(p, g, exc, match):
        p.grad = g
        opt = Adam([good, p])
        with pytest.raises(exc, match=match):
            opt.step()
        assert len(opt.state[good]) == 0 and bool((good == 0).all())     # refused before anything ran

    half = torch.nn.Parameter(torch.zeros(8, device=DEV, dtype=torch.float16))
    refused(half, torch.ones(8, device=DEV, dtype=torch.float16), ValueError, "parameter 1 .*float32")
    emb = torch.nn.Parameter(torch.zeros(4, 2, device=DEV))
    sparse = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.ones(1, 2), (4, 2)).to(DEV)
    refused(emb, sparse, ValueError, "parameter 1 .*sparse")
    gappy = torch.nn.Parameter(torch.zeros(8, 4, device=DEV)[:, :2])
    refused(gappy, torch.zeros(8, 4, device=DEV)[:, :2], ValueError, "parameter 1 .*not dense")
    mat = torch.nn.Parameter(torch.zeros(4, 6, device=DEV))
    refused(mat, torch.ones(6, 4, device=DEV).t(), ValueError, "parameter 1.*strides")


def test_step_reaches_the_field():
    """As test_fused_optimizer_step_reaches_the_field (tests/test_gpu_train.py): the kernel writes the parameters
    without advancing their version counters; the optimizer-step generation in FusedField's cache keys advances
    once per step, so the fused forward after each of 3 large steps equals PyTorch's forward of the same module."""
    import avr.field
    from avr.optim import Adam
    from avr.scene import synthetic_scene
    from helpers import model_conf
    net = synthetic_scene(DEV, 0, model_conf(64, 3, 1000, 64), latent_hw=(8, 8))
    for p in net.parameters():
        p.requires_grad_(True)
    g = torch.Generator(device="cpu").manual_seed(29)
    xyz = ((torch.rand(1, 300, 3, generator=g) - 0.5) * 0.8).to(DEV)
    vd = torch.nn.functional.normalize(torch.randn(1, 300, 3, generator=g), dim=-1).to(DEV)
    w = torch.randn(1, 300, 4, generator=g).to(DEV)
    opt = Adam(net.mlp_coarse.parameters(), lr=5e-2)
    for _ in range(3):
        opt.zero_grad()
        out = net(xyz, coarse=True, viewdirs=vd)
        with torch.no_grad():
            ref = net.forward_torch(xyz, True, vd)
        np.testing.assert_allclose(_np(out), _np(ref), atol=1e-4)
        (out * w).sum().backward()
        gen = avr.field.param_generation()
        before = net.mlp_coarse.lin_out.weight.detach().clone()
        versions = [p._version for p in net.mlp_coarse.parameters()]
        opt.step()
        assert avr.field.param_generation() == gen + 1
        assert versions == [p._version for p in net.mlp_coarse.parameters()]
        assert not torch.equal(before, net.mlp_coarse.lin_out.weight)
    with torch.no_grad():
        assert net.can_fuse(xyz)
        a = net(xyz, coarse=True, viewdirs=vd)
        b = net.forward_torch(xyz, True, vd)
    np.testing.assert_allclose(_np(a), _np(b), atol=1e-4)


def test_graphed_train_step_with_avr_adam_matches_eager(monkeypatch):
    """The body of test_graphed_train_step_matches_eager_adaptive (tests/test_gpu_graphs.py) with avr.optim.Adam
    constructed without flags: the captured step's 6 losses and every parameter equal the eager run's bit for bit,
    in one capture (the marched point's pass on the capturing stream: one branch)."""
    from test_gpu_poison import _setup
    from avr.graphs import GraphedTrainStep
    from avr.optim import Adam
    monkeypatch.setenv("AVR_ADAPTIVE_SIDE_STREAM_IN_GRAPH", "0")
    runs = []
    for graphed in (False, True):
        net, rend, named, (c2w, K, x_pix, gt), _ = _setup("adaptive", False)
        opt = Adam([p for _, p in named], lr=1e-4)

        def step():
            rgb_c, rgb_f, _, _ = rend(c2w, K, x_pix, net)
            loss = ((rgb_c - gt) ** 2).mean() + ((rgb_f - gt) ** 2).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss
        run = GraphedTrainStep(step, nets=[net], renderers=[rend], warmup=2) if graphed else step
        torch.manual_seed(123)
        losses = [float(run()) for _ in range(6)]
        assert rend.last_path == "hip_train"
        if graphed:
            assert run.captures == 1 and run.calls == 6
        runs.append((losses, {n: p.detach().clone() for n, p in named}))
    (le, pe), (lg, pg) = runs
    assert all(torch.isfinite(torch.tensor(le)))
    assert le == lg, (le, lg)
    for n in pe:
        assert torch.equal(pe[n], pg[n]), n
