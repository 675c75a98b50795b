"""avr.cache on the CPU (no GPU, no library call): the one cache record and lookup (_Record, _cached), the join rule
of _stamp / _join eagerly and inside a capture scope (against fakes of the three torch.cuda names the module uses),
the generation counters' hooks, and the adaptive renderers' gate tables, which go through the same protocol."""
import gc
import types
import weakref

import pytest
import torch

from avr import cache


class _Held:
    """Something weakly referenceable for a record's keep field."""


def test_cached_builds_once_per_key_and_releases_the_old_keep():
    store, made = {}, []

    def make():
        made.append(torch.zeros(3))
        return made[-1]

    keep = _Held()
    dead = weakref.ref(keep)
    a = cache._cached(store, "slot", ("k", 1), make, keep=keep)
    assert cache._cached(store, "slot", ("k", 1), make, keep=keep) is a and len(made) == 1
    rec = store["slot"]
    assert (rec.key, rec.keep) == (("k", 1), keep) and rec.value is a and rec[0] == rec.key and rec[1] is a
    # a CPU tensor: nothing to stamp, and the join of a stampless record is a no-op
    assert rec.stamp is None and cache._stamp(a) is None
    cache._join(rec.stamp, rec.value)
    del keep, rec
    b = cache._cached(store, "slot", ("k", 2), make, keep=_Held())
    assert b is not a and len(made) == 2 and store["slot"].key == ("k", 2)
    gc.collect()
    assert dead() is None                       # the replaced entry's keep went with it
    # another slot of the same store is its own entry; a host-side value (device=False) is never stamped
    v = cache._cached(store, "other", ("k", 2), lambda: object(), device=False)
    assert cache._cached(store, "other", ("k", 2), lambda: object(), device=False) is v
    assert store["other"].stamp is None and store["slot"].value is b


def test_cached_stamps_and_joins_the_tensor_of_the_value_it_is_told():
    """of: which tensor of a composite value the record's stamp marks (FusedField.packed: the blob of a _Packed)."""
    seen = []
    value = types.SimpleNamespace(packed=torch.zeros(2))
    store = {}
    of = lambda v: seen.append(v) or v.packed  # noqa: E731
    assert cache._cached(store, 0, "k", lambda: value, of=of) is value and seen == [value]
    assert cache._cached(store, 0, "k", lambda: None, of=of) is value and seen == [value, value]
    assert store[0].stamp is None


# ------------------------------------------------------------------------------------------------- the join rule
class _Stream:
    def __init__(self, name):
        self.name, self.device, self.waited = name, "dev0", []

    def wait_event(self, event):
        self.waited.append(event)


class _Event:
    def __init__(self):
        self.recorded_on = []

    def record(self, stream):
        self.recorded_on.append(stream)


class _DeviceTensor:
    is_cuda, device = True, "dev0"

    def __init__(self):
        self.recorded = []

    def record_stream(self, stream):
        self.recorded.append(stream)


@pytest.fixture
def cuda(monkeypatch):
    """What avr.cache sees of torch.cuda: is_current_stream_capturing, current_stream, Event. The test sets
    `capturing` and `stream`."""
    fake = types.SimpleNamespace(capturing=False, stream=_Stream("main"), Event=_Event)
    fake.is_current_stream_capturing = lambda: fake.capturing
    fake.current_stream = lambda device=None: fake.stream
    monkeypatch.setattr(cache, "torch", types.SimpleNamespace(cuda=fake))
    return fake


def _counting(value):
    made = []

    def make():
        made.append(1)
        return value
    return make, made


def test_join_rule_eager(cuda):
    main, side = cuda.stream, _Stream("side")
    t = _DeviceTensor()
    make, made = _counting(t)
    store = {}
    assert cache._cached(store, 0, "k", make) is t
    stream, event, scope = store[0].stamp
    assert stream is main and scope == 0 and event.recorded_on == [main]
    # a hit on the maker's stream neither waits nor records
    assert cache._cached(store, 0, "k", make) is t
    assert main.waited == [] and t.recorded == []
    # a hit on another stream waits once for the maker's event and records that stream once
    cuda.stream = side
    assert cache._cached(store, 0, "k", make) is t
    assert side.waited == [event] and t.recorded == [side] and main.waited == [] and made == [1]
    # an eager stamp read under a capture (inside a scope or not) is joined too
    cuda.capturing = True
    with cache.capture_scope():
        cache._cached(store, 0, "k", make)
    cache._cached(store, 0, "k", make)
    assert side.waited == [event] * 3 and made == [1]


def test_join_rule_inside_a_capture_scope(cuda):
    main, side = cuda.stream, _Stream("side")
    t = _DeviceTensor()
    make, made = _counting(t)
    store = {}
    cuda.capturing = True
    with cache.capture_scope() as k:
        assert k != 0 and cache._SCOPE[0] == k
        cuda.stream = side                               # made on the graph's side stream
        assert cache._cached(store, 0, "k", make) is t
        stream, event, scope = store[0].stamp
        assert stream is side and scope == k and event.recorded_on == [side]
        assert cache._cached(store, 0, "k", make) is t    # its own stream: no wait
        assert side.waited == [] and t.recorded == []
        cuda.stream = main                               # read on the capturing stream: the graph edge
        assert cache._cached(store, 0, "k", make) is t
        assert main.waited == [event] and t.recorded == [main]
    assert cache._SCOPE[0] == 0
    # the same record after the scope ended (eagerly, and in a scopeless capture), and inside the next scope:
    # the value with no wait -- the event belongs to a capture that is over
    cuda.capturing = False
    assert cache._cached(store, 0, "k", make) is t
    cuda.capturing = True
    assert cache._cached(store, 0, "k", make) is t
    with cache.capture_scope() as k2:
        assert k2 not in (0, k)
        assert cache._cached(store, 0, "k", make) is t
    assert main.waited == [event] and t.recorded == [main] and made == [1]


def test_capture_without_a_scope_is_not_stamped_and_the_scope_ends_with_an_exception(cuda):
    cuda.capturing = True
    t = _DeviceTensor()
    store = {}
    assert cache._cached(store, 0, "k", lambda: t) is t and store[0].stamp is None
    assert cache._stamp(t) is None and cache._stamp(None) is None
    with pytest.raises(RuntimeError, match="inside"):
        with cache.capture_scope() as k:
            assert cache._SCOPE[0] == k != 0 and cache._stamp(t)[2] == k
            raise RuntimeError("inside")
    assert cache._SCOPE[0] == 0 and cache._stamp(t) is None


# ------------------------------------------------------------------------------------------------- the counters
def test_the_optimizer_hook_is_registered_once_whatever_is_imported_first():
    """avr.field, avr.renderers and avr.graphs read avr.cache's counters: one module, one hook, one count per
    optimizer step (avr.field's names are the same functions)."""
    import importlib
    for names in (("avr.field", "avr.cache"), ("avr.cache", "avr.field"), ("avr.graphs", "avr.renderers")):
        mods = [importlib.import_module(n) for n in names]
        assert all(getattr(m, "param_generation", cache.param_generation) is cache.param_generation for m in mods)
    from avr import field
    assert field.bump_param_generation is cache.bump_param_generation
    p = torch.nn.Parameter(torch.ones(2))
    opt = torch.optim.SGD([p], lr=0.1)
    p.grad = torch.ones(2)
    g0, e0 = cache.param_generation(), cache._EXPLICIT_GEN[0]
    opt.step()
    assert field.param_generation() == g0 + 1 and cache._EXPLICIT_GEN[0] == e0
    field.bump_param_generation()
    assert cache.param_generation() == g0 + 2 and cache._EXPLICIT_GEN[0] == e0 + 1
    m0 = cache._MODULE_GEN[0]
    torch.nn.Sequential().add_module("lin", torch.nn.Identity())
    assert cache._MODULE_GEN[0] == m0 + 1


# ------------------------------------------------------------------------------------------------- gate tables
def _march(sb, seed=3):
    from avr.renderers import _LSTMMarch
    g = torch.Generator().manual_seed(seed)
    march = _LSTMMarch(16, 2)
    phi = types.SimpleNamespace(encoder=types.SimpleNamespace(latent=torch.randn(sb, 16, 4, 4, generator=g)))
    return march, phi


def _product(march, lat_s):
    return torch.matmul(lat_s.detach().reshape(16, -1).t().float(), march.lstm.weight_ih.detach().t().float())


def test_gate_tables_are_the_per_scene_products_cached_per_scene_count():
    march, phi = _march(1)
    assert march.cache_tensors() == []
    one = march._gate_tables(phi, 1)
    assert one.shape == (1, 16, 64) and torch.equal(one[0], _product(march, phi.encoder.latent[0]))
    assert march._gate_tables(phi, 1) is one                       # a hit: the same tensor object
    three = march._gate_tables(phi, 3)                             # one map for three scenes: repeated
    assert three.shape == (3, 16, 64) and three.is_contiguous() and all(torch.equal(three[s], one[0]) for s in range(3))
    assert march._gate_tables(phi, 3) is three and march._gate_tables(phi, 1) is one
    assert {id(t) for t in march.cache_tensors()} == {id(one), id(three)}   # every slot in use
    rec = march._gates[3]
    assert rec.keep[0] is phi.encoder.latent and rec.keep[1] is march.lstm.weight_ih and rec.stamp is None

    march3, phi3 = _march(3)
    own = march3._gate_tables(phi3, 3)                             # a map per scene: three different tables
    for s in range(3):
        assert torch.equal(own[s], _product(march3, phi3.encoder.latent[s]))
    assert not torch.equal(own[0], own[1]) and not torch.equal(own[1], own[2])
    assert torch.equal(march3._gate_tables(phi3, 1)[0], own[0])    # one scene of several maps: scene 0's


def test_gate_tables_are_rebuilt_after_a_weight_write_and_a_generation_bump():
    march, phi = _march(1)
    first = march._gate_tables(phi, 1)
    with torch.no_grad():
        march.lstm.weight_ih.mul_(0.5)                             # in place: the version counter sees it
    second = march._gate_tables(phi, 1)
    assert second is not first and torch.equal(second[0], _product(march, phi.encoder.latent[0]))
    assert not torch.equal(second, first) and march._gate_tables(phi, 1) is second
    cache.bump_param_generation()                                  # an update no counter records
    third = march._gate_tables(phi, 1)
    assert third is not second and torch.equal(third, second) and march.cache_tensors()[0] is third
    with torch.no_grad():
        phi.encoder.latent.add_(1.0)                               # the latent's version is in the key too
    assert march._gate_tables(phi, 1) is not third
