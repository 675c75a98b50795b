"""avr.field._FieldTrain's weight-gradient layer list on the CPU (no GPU): which launch position every named
gradient comes from, and which rows each position reads. avr.ops.weight_grads_specs is replaced by a fake that
returns, for layer k of the launch, tensors of the layer's shapes filled with k. The kernels and the gradients'
values are held to float64 on the MI355X (tests/test_gpu_train.py)."""
import pytest
import torch

from avr import _lib, field, ops

NB, H, D_LATENT, NUM_FREQS, MT = 3, 64, 128, 6, 10
D_IN = 6 * NUM_FREQS + 6
ZS = D_IN + (-D_IN) % 4


@pytest.mark.parametrize("combine_layer", [2, 1000])
def test_field_train_weight_grads_by_name(monkeypatch, combine_layer):
    nz = min(combine_layer, NB)
    dims = _lib.FieldDims(D_IN, D_LATENT, H, NB, nz, NUM_FREQS, 1.5, _lib.FIELD_X3, 0, 0, 0.0)
    n_l = 2 * NB + 1
    G, act = torch.zeros(n_l, MT, H), torch.zeros(n_l, MT, H)
    g_max, act_max = torch.zeros(n_l, dtype=torch.int32), torch.zeros(n_l + 1, dtype=torch.int32)
    lat_feat, lat_max = torch.zeros(MT, D_LATENT), torch.zeros(1, dtype=torch.int32)
    zf, d4, d4_max = torch.zeros(MT, ZS), torch.zeros(MT, 4), torch.zeros(1, dtype=torch.int32)
    launches = []

    def weight_grads_specs(specs, n_rows, dev, stream, n_split=None):
        launches.append((specs, n_rows))
        return [(torch.full((s[4], s[5]), float(k)), torch.full((s[4],), float(k)) if s[8] else None)
                for k, s in enumerate(specs)]

    monkeypatch.setattr(ops, "weight_grads_specs", weight_grads_specs)
    monkeypatch.setattr(field, "stream_of", lambda t: None)
    grads = field._weight_grads(dims, MT, G, g_max, act, act_max, lat_feat, lat_max, zf, d4, d4_max)

    (specs, n_rows), = launches                               # one launch over all the rows
    assert n_rows == MT and len(specs) == 2 * NB + nz + 2
    position = {}
    for b in range(NB):
        position[f"blocks.{b}.fc_0"], position[f"blocks.{b}.fc_1"] = 2 * b, 2 * b + 1
    for b in range(nz):
        position[f"lin_z.{b}"] = 2 * NB + b
    position["lin_in"], position["lin_out"] = 2 * NB + nz, 2 * NB + nz + 1
    assert set(grads) == {n + e for n in position for e in (".weight", ".bias")}
    for name, k in position.items():
        assert bool((grads[name + ".weight"] == k).all()), name
        if not name.startswith("lin_z"):
            assert bool((grads[name + ".bias"] == k).all()), name
    # lin_z[b] asks for no bias gradient: its output gradient is the one at block b's input
    for b in range(nz):
        assert specs[position[f"lin_z.{b}"]][8] is False
        assert grads[f"lin_z.{b}.bias"] is (grads[f"blocks.{b - 1}.fc_1.bias"] if b > 0 else grads["lin_in.bias"])
    assert grads["lin_in.weight"].shape == (H, D_IN) and grads["lin_in.weight"].is_contiguous()
    assert specs[position["lin_in"]][5] == ZS                  # (the launch's operand rows are padded to 16 B)
    assert grads["lin_out.weight"].shape == (4, H) and grads["lin_z.0.weight"].shape == (H, D_LATENT)
    # the rows each position contracts: (gradient, input) addresses
    rows = {f"blocks.{k // 2}.fc_{k % 2}": (G[k], act[k]) for k in range(2 * NB)}
    rows.update({f"lin_z.{b}": (G[2 * b - 1] if b > 0 else G[2 * NB], lat_feat) for b in range(nz)})
    rows.update(lin_in=(G[2 * NB], zf), lin_out=(d4, act[2 * NB]))
    for name, (g, x) in rows.items():
        s = specs[position[name]]
        assert (s[0], s[2]) == (g.data_ptr(), x.data_ptr()), name
