"""avr.field's cache bookkeeping on the CPU (no GPU, no library call): the one cache record and lookup (_Record,
_cached), a packed blob's by-value dims per kernel precision (_Packed.dims_as), the multi-scene launches' groups
(scene_groups) and what FusedField.cache_tensors() hands a captured graph."""
import gc
import weakref

import pytest
import torch

from avr import _lib, field


def _dims(precision=_lib.FIELD_X3):
    return _lib.FieldDims(42, 64, 64, 2, 2, 6, 1.5, precision, 0, 0, 0.0)


class _Held:
    """Something weakly referenceable for a record's keep field."""


def test_cached_builds_once_per_key_and_releases_the_old_keep():
    store, made = {}, []

    def make():
        made.append(torch.zeros(3))
        return made[-1]

    keep = _Held()
    dead = weakref.ref(keep)
    a = field._cached(store, "slot", ("k", 1), make, keep=keep)
    assert field._cached(store, "slot", ("k", 1), make, keep=keep) is a and len(made) == 1
    rec = store["slot"]
    assert (rec.key, rec.keep) == (("k", 1), keep) and rec.value is a and rec[0] == rec.key and rec[1] is a
    # a CPU tensor: nothing to stamp, and the join of a stampless record is a no-op
    assert rec.stamp is None and field._stamp(a) is None
    field._join(rec.stamp, rec.value)
    del keep, rec
    b = field._cached(store, "slot", ("k", 2), make, keep=_Held())
    assert b is not a and len(made) == 2 and store["slot"].key == ("k", 2)
    gc.collect()
    assert dead() is None                       # the replaced entry's keep went with it
    # another slot of the same store is its own entry; a host-side value (device=False) is never stamped
    v = field._cached(store, "other", ("k", 2), lambda: object(), device=False)
    assert field._cached(store, "other", ("k", 2), lambda: object(), device=False) is v
    assert store["other"].stamp is None and store["slot"].value is b


@pytest.mark.parametrize("packed_as", [_lib.FIELD_X3, _lib.FIELD_FP32])
def test_packed_dims_as_are_copies_differing_in_precision_only(packed_as):
    dims = _dims(packed_as)
    entry = field._Packed(dims, torch.zeros(4))
    assert entry.dims is dims and entry.bwd is None and entry.tables == {} and entry.batch_tables == {}
    assert entry.weights is None and entry.keep is None
    off, size = _lib.FieldDims.precision.offset, _lib.FieldDims.precision.size
    snap = bytes(entry.dims)
    for precision in (_lib.FIELD_X3, _lib.FIELD_FP32):
        copy = entry.dims_as(precision)
        assert copy is not entry.dims and isinstance(copy, _lib.FieldDims) and copy.precision == precision
        assert copy is entry.dims_as(precision)                  # made once, at pack time
        got = bytes(copy)
        assert got[:off] == snap[:off] and got[off + size:] == snap[off + size:]
    assert entry.dims_as(_lib.FIELD_X3) is not entry.dims_as(_lib.FIELD_FP32)
    fresh = entry.dims.with_precision(_lib.FIELD_X3)             # the copy helper itself: a new struct per call
    assert fresh is not entry.dims_as(_lib.FIELD_X3) and bytes(fresh) == bytes(entry.dims_as(_lib.FIELD_X3))
    entry.dims_as(_lib.FIELD_X3).d_hidden = 128                  # a write to a copy stays in the copy
    entry.dims_as(_lib.FIELD_FP32).precision = 7
    assert bytes(entry.dims) == snap and entry.dims.d_hidden == 64 and entry.dims.precision == packed_as


@pytest.mark.parametrize("n", [0, 1, _lib.AVR_MAX_SCENES, _lib.AVR_MAX_SCENES + 1, 3 * _lib.AVR_MAX_SCENES])
def test_scene_groups_tile_the_scenes(n):
    groups = list(field.scene_groups(n))
    assert all(1 <= count <= _lib.AVR_MAX_SCENES for _, count in groups)
    assert [s for g0, count in groups for s in range(g0, g0 + count)] == list(range(n))
    assert len(groups) == -(-n // _lib.AVR_MAX_SCENES)


def test_cache_tensors_walks_the_declared_fields():
    fused = field.FusedField(net=None)
    blob, bwd, table, batch = (torch.zeros(2) for _ in range(4))
    entry = field._Packed(_dims(), blob)
    entry.bwd = field._Record(None, bwd)
    entry.tables[0] = field._Record(("t",), table)
    entry.batch_tables[True] = field._Record(("b",), batch)
    fused._packed[True] = field._Record(("key",), entry)
    fused._packed[False] = (("stale",), None)                    # planted by hand (tests/test_parallel_cpu.py)
    got = fused.cache_tensors()
    assert len(got) == 4 and {id(t) for t in got} == {id(blob), id(bwd), id(table), id(batch)}
    fused.invalidate()
    assert not fused._packed and fused.cache_tensors() == []
