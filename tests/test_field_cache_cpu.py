"""avr.field's cache bookkeeping on the CPU (no GPU, no library call; the protocol itself: tests/test_cache_cpu.py):
a packed blob's by-value dims per kernel precision (_Packed.dims_as), the multi-scene launches' groups
(scene_groups), what FusedField.cache_tensors() hands a captured graph, and the key of the latent map's copies."""
import pytest
import torch

from avr import _lib, field


def _dims(precision=_lib.FIELD_X3):
    return _lib.FieldDims(42, 64, 64, 2, 2, 6, 1.5, precision, 0, 0, 0.0)


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


def _latent_rebuilds(latent, change):
    """How often FusedField._latent_cached rebuilds a copy of `latent` over: a call, a repeat, change(), a call."""
    fused = field.FusedField(net=None)
    made = []

    def get():
        return fused._latent_cached("copy", latent, lambda: made.append(1) or latent.detach().clone())
    first = get()
    assert get() is first and len(made) == 1
    change()
    after = get()
    assert (after is first) == (len(made) == 1)
    return len(made) - 1, after


def _fused_adam_step(leaf):
    """A step that updates the leaf's storage without advancing any version counter (torch's fused Adam)."""
    opt = torch.optim.Adam([leaf], lr=0.1, fused=True)
    leaf.grad = torch.ones_like(leaf)

    def step():
        versions = leaf._version
        opt.step()
        assert leaf._version == versions
    return step


def test_latent_copies_of_a_view_of_a_trainable_leaf_follow_the_optimizer():
    """encoder.latent = param[idx] shares the leaf's storage: the optimizer-step count is in its key, as for the
    leaf itself."""
    leaf = torch.nn.Parameter(torch.ones(4, 16, 2, 2))
    view = leaf[1:3]
    assert not view.is_leaf and view._base is leaf
    rebuilt, after = _latent_rebuilds(view, _fused_adam_step(leaf))
    assert rebuilt == 1 and torch.equal(after, view.detach()) and not torch.equal(after, torch.ones(2, 16, 2, 2))
    assert _latent_rebuilds(leaf, _fused_adam_step(leaf))[0] == 1


def test_latent_copies_of_a_fixed_map_outlive_optimizer_steps_but_not_a_generation_bump():
    plain = torch.ones(2, 16, 2, 2) * 2.0            # an encoder's output: no leaf that requires grad behind it
    assert plain._base is None and not plain.requires_grad
    other = torch.nn.Parameter(torch.ones(3))
    assert _latent_rebuilds(plain, _fused_adam_step(other))[0] == 0
    produced = (torch.nn.Parameter(torch.ones(2, 16, 2, 2)) * 2.0)   # a non-leaf with history, not a view
    assert not produced.is_leaf and produced._base is None
    assert _latent_rebuilds(produced, _fused_adam_step(other))[0] == 0
    assert _latent_rebuilds(plain, field.bump_param_generation)[0] == 1
