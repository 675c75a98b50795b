"""The cache protocol of avr.field, avr.renderers and avr.graphs, and the process-wide counters its keys are built
from. Every cache entry is one _Record(key, value, keep, stamp) behind _cached: a hit under the same key joins the
reading stream to the maker's (_join), a miss builds, stamps (_stamp) and stores. _stamp and _join alone touch
streams and events for a cached value; capture_scope() names the HIP-graph capture in progress, so that a value
made inside a capture is stream-ordered inside it and never waited for after it."""
import collections
import contextlib
import typing

import torch
from torch.optim.optimizer import register_optimizer_step_post_hook

# Submodule (re)registrations anywhere in the process, numbered, with the id of the module that registered: a
# FusedField._state slot is rebuilt after a registration under its MLP, so a module replaced in an MLP
# (mlp.lin_in = nn.Linear(...)) is seen, and only then (modules built elsewhere, e.g. per training step, leave it
# alone); parameters and buffers replaced in place are read through their owners' dicts anyway.
_MODULE_GEN = [0]
_REG_LOG = collections.deque(maxlen=4096)   # (generation, id(parent module))


def _module_registered(module, name, submodule):
    _MODULE_GEN[0] += 1
    _REG_LOG.append((_MODULE_GEN[0], id(module)))


def _slot_current(gen, module_ids):
    """No registration since generation `gen` under a module of module_ids (the log must still cover them all;
    a reused id only costs a rebuild)."""
    if gen == _MODULE_GEN[0]:
        return True
    if not _REG_LOG or _REG_LOG[0][0] > gen + 1:
        return False
    return not any(pid in module_ids for g, pid in _REG_LOG if g > gen)


torch.nn.modules.module.register_module_module_registration_hook(_module_registered)


# Every optimizer step anywhere in the process, counted: a fused optimizer (torch.optim.Adam(fused=True)) updates
# the parameters in one multi-tensor kernel without advancing their version counters, so the (data_ptr, _version)
# keys of the caches would not see it (the blob would keep the old weights). The count is part of every key;
# GraphedTrainStep advances it after each replay (a captured optimizer step runs no host hook).
_PARAM_GEN = [0]
_EXPLICIT_GEN = [0]   # bump_param_generation() calls alone: the key of latent maps no optimizer can hold


def _optimizer_stepped(optimizer, args, kwargs):
    _PARAM_GEN[0] += 1


register_optimizer_step_post_hook(_optimizer_stepped)


def bump_param_generation():
    """Invalidate every cache entry derived from parameters or the latent map (after an update the version
    counters do not record: a replayed optimizer step, a write through .data)."""
    _PARAM_GEN[0] += 1
    _EXPLICIT_GEN[0] += 1


def param_generation():
    return _PARAM_GEN[0]


def _version_key(tensors, gen=True):
    """(data_ptr, _version) of each tensor, with the optimizer-step generation for anything an optimizer may
    update (gen=False: the source views -- poses, focal, principal point -- which none does)."""
    return ((_PARAM_GEN[0],) if gen else ()) + tuple((t.data_ptr(), t._version) for t in tensors)


_SCOPE = [0, 0]   # [id of the HIP-graph capture in progress (0: none, eager), the last id handed out]


@contextlib.contextmanager
def capture_scope():
    """Around a torch.cuda.graph(...) block (avr.graphs): the capture gets a fresh non-zero id, which the stamps made
    inside it carry; 0 again on the way out, also by an exception. Process wide, not thread local: the autograd
    engine's device thread stamps and joins the backward's values under it."""
    _SCOPE[0] = _SCOPE[1] = _SCOPE[1] + 1
    try:
        yield _SCOPE[0]
    finally:
        _SCOPE[0] = 0


def _stamp(t):
    """(stream, event, scope) marking the current stream's work that filled the cached device tensor t. scope is 0
    for an eager value and the capture_scope() id for one made inside that capture (an event record on a capturing
    stream is legal; a wait for it is the graph edge from the maker to a reader on the graph's other stream). None
    on the CPU and in a capture outside any scope (a caller's own torch.cuda.graph): read without a join."""
    if t is None or not t.is_cuda:
        return None
    capturing = torch.cuda.is_current_stream_capturing()
    if capturing and not _SCOPE[0]:
        return None
    s = torch.cuda.current_stream(t.device)
    ev = torch.cuda.Event()
    ev.record(s)
    return s, ev, _SCOPE[0] if capturing else 0


def _join(stamp, *tensors):
    """A cached value read from another stream than its maker's (the adaptive renderer's side stream): that stream
    waits for the maker's work, and the tensors' memory is kept from reuse under the maker's later allocations until
    this stream's work on them is done. So for eager stamps, read eagerly or under a capture, and for stamps of the
    capture in progress; a stamp of another capture (it has ended: waiting for its event is an error) is read
    without a wait, as a stampless value is."""
    if stamp is None or (stamp[2] and stamp[2] != _SCOPE[0]):
        return
    s = torch.cuda.current_stream(stamp[0].device)
    if s == stamp[0]:
        return
    s.wait_event(stamp[1])
    for t in tensors:
        if t is not None and t.is_cuda:
            t.record_stream(s)


class _Record(typing.NamedTuple):
    """One cache entry: the comparable key it was built under, the value, whatever must stay alive for the key
    to stay sound (a tensor whose address is part of it), and the _stamp of the value's maker."""
    key: object
    value: object
    keep: object = None
    stamp: object = None


def _hit(rec, key, of=None):
    """True when rec holds a value built under `key`; the current stream is then joined to its maker's."""
    if rec is None or rec.key != key:
        return False
    _join(rec.stamp, rec.value if of is None else of(rec.value))
    return True


def _cached(store, slot, key, make, keep=None, device=True, of=None):
    """store[slot]'s value if it was built under `key`, else make() stored in its place (the cache protocol of
    every cache here; device=False: a host-side value, nothing to stamp or join; of: value -> the device tensor
    of it to stamp and join, the value itself by default)."""
    rec = store.get(slot)
    if not _hit(rec, key, of):
        value = make()
        rec = store[slot] = _Record(key, value, keep, _stamp(value if of is None else of(value)) if device else None)
    return rec.value
