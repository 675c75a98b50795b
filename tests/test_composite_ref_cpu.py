"""tests/composite_ref.py is not self-made truth: its float64 forward against the oracle and the golden vectors, its
gradients against the modelled project's recorded autograd and against central differences of its own forward, its
march against the forward it truncates; and the conditions the GPU march tests put on their inputs. CPU only."""
import itertools

import numpy as np
import pytest
import torch

import composite_ref as C
from oracle import avr_oracle as O

F64 = torch.float64
GOLDEN_CASES = [(N, wb) for N in (64, 128, 192) for wb in (0, 1)]


def _golden_case(golden, N, wb):
    g = golden("g1_volume_integral.npz")
    k = f"N{N}_wb{wb}"
    z = torch.from_numpy(g[f"{k}_z"][0])
    field = torch.from_numpy(np.concatenate([g[f"{k}_rad"][0], g[f"{k}_sigma"][0]], -1))
    return g, k, z, field


@pytest.mark.parametrize("N,wb", GOLDEN_CASES)
def test_forward_matches_oracle_and_golden(golden, N, wb):
    """2e-6 absolute on rgb, depth and weights: the bound the GPU forward tests hold the kernel to."""
    g, k, z, field = _golden_case(golden, N, wb)
    rgb, dist, w = (t.numpy() for t in C.volume_integral(z, field, bool(wb)))
    orgb, odep, ow = O.volume_integral(g[f"{k}_z"], g[f"{k}_sigma"], g[f"{k}_rad"], bool(wb))
    for name, got, ora, gold in (("rgb", rgb, orgb[0], g[f"{k}_rgb"][0]),
                                 ("depth", dist, odep[0, :, 0], g[f"{k}_depth"][0, :, 0]),
                                 ("weights", w, ow[0, ..., 0], g[f"{k}_weights"][0, ..., 0])):
        print(f"{k} {name}: vs oracle {np.abs(got - ora).max():.2e}, vs golden {np.abs(got - gold).max():.2e}")
        np.testing.assert_allclose(got, ora, atol=2e-6, rtol=0, err_msg=name)
        np.testing.assert_allclose(got, gold, atol=2e-6, rtol=0, err_msg=name)


@pytest.mark.parametrize("N,wb", GOLDEN_CASES)
def test_grads_match_golden_autograd(golden, N, wb):
    """The float64 gradients against the modelled project's own fp32 autograd: drad to 2e-6, dsigma[:, :N-1] to 2e-5
    of max(|ref|, 1), and the last column (see composite_ref's docstring) as one array, within twice the error of
    this module's fp32 autograd plus one fp32 epsilon of its largest entry."""
    g, k, z, field = _golden_case(golden, N, wb)
    g_rgb, g_dist = torch.from_numpy(g[f"{k}_grad_rgb"][0]), torch.from_numpy(g[f"{k}_grad_depth"][0, :, 0])
    gf, _ = C.grads(z, field, g_rgb, g_dist, None, bool(wb))
    gf = gf.numpy()
    drad, dsig = g[f"{k}_drad"][0].astype(np.float64), g[f"{k}_dsigma"][0, ..., 0].astype(np.float64)
    e_rad = np.abs(gf[..., :3] - drad).max()
    scale = np.maximum(np.abs(dsig[:, :-1]), 1.0)
    e_sig = (np.abs(gf[:, :-1, 3] - dsig[:, :-1]) / scale).max()
    g32, _ = C.grads(z, field, g_rgb, g_dist, None, bool(wb), dtype=torch.float32)
    last64, last32 = gf[:, -1, 3], g32[:, -1, 3].double().numpy()
    e_last, e_base = np.abs(dsig[:, -1] - last64).max(), np.abs(last32 - last64).max()
    bound = 2.0 * e_base + C.EPS32 * np.abs(last64).max()
    print(f"{k}: drad {e_rad:.2e}, dsigma[:, :N-1] {e_sig:.2e} of max(|ref|, 1), dsigma[:, N-1] golden {e_last:.3e} "
          f"fp32 {e_base:.3e} bound {bound:.3e} max {np.abs(last64).max():.3e}")
    assert e_rad <= 2e-6
    assert e_sig <= 2e-5
    assert e_last <= bound


def test_last_column_fact(golden):
    """The figures of composite_ref's docstring."""
    g, k, z, field = _golden_case(golden, 192, 1)
    g_rgb, g_dist = torch.from_numpy(g[f"{k}_grad_rgb"][0]), torch.from_numpy(g[f"{k}_grad_depth"][0, :, 0])
    gf, _ = C.grads(z, field, g_rgb, g_dist, None, True)
    assert float(field[3, -1, 3]) == 0.0
    assert abs(float(gf[3, -1, 3]) - (-2.287)) < 1e-3
    assert abs(float(g[f"{k}_dsigma"][0, 3, -1, 0]) - (-1.769)) < 1e-3


@pytest.mark.parametrize("wb", [False, True])
@pytest.mark.parametrize("with_dist,with_w", list(itertools.product([True, False], repeat=2)))
def test_grads_match_central_differences(wb, with_dist, with_w):
    """Every coordinate of z, sigma and rgb of two rays at N = 5 against central differences (h = 1e-5) of the float64
    forward, the loss written out here with the g_dist and g_w terms present or not: a term that grads drops, or keeps
    where its gradient is None, is an O(1) error. Truncation h^2 f''' / 6 is below 1e-8 (|sigma| <= 4, |g| <= 3 or
    so) and rounding 2^-52 |loss| / h below 1e-10; the bound is 1e-7 of max(|g|, 1)."""
    gen = torch.Generator().manual_seed(11)
    R, N, h = 2, 5, 1e-5
    z = torch.sort(0.8 + torch.rand(R, N, generator=gen, dtype=F64), -1)[0]
    field = torch.cat([torch.rand(R, N, 3, generator=gen, dtype=F64),
                       0.5 + 3.5 * torch.rand(R, N, 1, generator=gen, dtype=F64)], -1)
    field[1, 2, 3] = 0.0
    g_rgb = torch.randn(R, 3, generator=gen, dtype=F64)
    g_dist = torch.randn(R, generator=gen, dtype=F64) if with_dist else None
    g_w = torch.randn(R, N, generator=gen, dtype=F64) if with_w else None

    def loss(zv, fv):
        rgb, dist, w = C.volume_integral(zv, fv, wb)
        out = (rgb * g_rgb).sum()
        if with_dist:
            out = out + (dist * g_dist).sum()
        if with_w:
            out = out + (w * g_w).sum()
        return float(out)

    gf, gz = C.grads(z, field, g_rgb, g_dist, g_w, wb)
    fd_z, fd_f = torch.zeros_like(z), torch.zeros_like(field)
    for idx in itertools.product(range(R), range(N)):
        zp, zm = z.clone(), z.clone()
        zp[idx] += h
        zm[idx] -= h
        fd_z[idx] = (loss(zp, field) - loss(zm, field)) / (2 * h)
        for ch in range(4):
            fp, fm = field.clone(), field.clone()
            fp[idx + (ch,)] += h
            fm[idx + (ch,)] -= h
            fd_f[idx + (ch,)] = (loss(z, fp) - loss(z, fm)) / (2 * h)
    for name, got, fd in (("d z", gz, fd_z), ("d field", gf, fd_f)):
        err = float(((got - fd).abs() / fd.abs().clamp_min(1.0)).max())
        print(f"wb {wb} g_dist {with_dist} g_w {with_w} {name}: {err:.2e}, largest {float(fd.abs().max()):.2e}")
        assert err <= 1e-7, name
        assert float(fd.abs().max()) > 1e-2, name
    if with_w:   # the term is live: without it the gradient is another one
        gf0, gz0 = C.grads(z, field, g_rgb, g_dist, None, wb)
        assert float((gf0 - gf).abs().max()) > 1e-2 and float((gz0 - gz).abs().max()) > 1e-2
    if with_dist:
        gf0, gz0 = C.grads(z, field, g_rgb, None, g_w, wb)
        assert float((gf0 - gf).abs().max()) > 1e-2 and float((gz0 - gz).abs().max()) > 1e-2


@pytest.mark.parametrize("chunk", [1, 16, 37, 64])
@pytest.mark.parametrize("wb", [False, True])
def test_march_without_stop_is_volume_integral(chunk, wb):
    z, field, *_ = C.ray_inputs(8, 100, 3.0, 5)
    rgb, dist, _ = C.volume_integral(z, field, wb)
    m_rgb, m_dist, consumed, margin = C.march(z, field, chunk, 0.0, wb)
    assert bool((consumed == 100).all()) and bool(torch.isinf(margin).all())
    torch.testing.assert_close(m_rgb, rgb, atol=1e-14, rtol=0)
    torch.testing.assert_close(m_dist, dist, atol=1e-14, rtol=0)


@pytest.mark.parametrize("wb", [False, True])
def test_march_stops_after_the_opaque_chunk(wb):
    """An opaque sample in chunk 1 (samples 16 .. 31): the ray is alive after chunk 0, stops after chunk 1 and returns
    the sums over samples 0 .. 31 alone; its neighbour without that sample runs to the end."""
    N, chunk = 100, 16
    z, field, *_ = C.ray_inputs(2, N, 0.0, 6)
    field[..., 3] = 0.3
    field[0, 20, 3] = 1e4
    rgb, dist, consumed, margin = C.march(z, field, chunk, 1e-3, wb)
    assert consumed.tolist() == [32, N]
    _, _, w = C.volume_integral(z, field, wb)
    zz = torch.cat([z[:, 1:], torch.full_like(z[:, :1], 1.8)], -1).double()
    want = (w[0, :32, None] * field[0, :32, :3].double()).sum(0) + (1.0 - w[0, :32].sum() if wb else 0.0)
    torch.testing.assert_close(rgb[0], want, atol=1e-14, rtol=0)
    torch.testing.assert_close(dist[0], (w[0, :32] * zz[0, :32]).sum(), atol=1e-14, rtol=0)
    full_rgb, full_dist, _ = C.volume_integral(z, field, wb)
    torch.testing.assert_close(rgb[1], full_rgb[1], atol=1e-14, rtol=0)
    # the margins: ray 0 was far above t_stop after chunk 0 and far below it after chunk 1
    assert float(margin[0]) > 0.5 and float(margin[1]) > 0.5


@pytest.mark.parametrize("N,chunk", C.MARCH_CASES)
def test_march_inputs_are_live_and_decided(N, chunk):
    """What the GPU march tests need of their inputs, on the reference alone: no ray within 1e-4 of a flipped decision
    (the tests allow 1 %), and rays that stop after the first chunk, rays that never stop and, where there is more
    than one boundary, rays that stop in between."""
    ro, rd, z = C.march_rays(C.MARCH_R, N, C.MARCH_SEED)
    field = C.march_field(ro, rd, z, C.march_amp(N))
    _, _, consumed, margin = C.march(z, field, chunk, C.MARCH_T_STOP, True)
    live = C.march_liveness(consumed, N, chunk)
    undecided = int((margin <= C.MARCH_MARGIN).sum())
    print(f"N {N} chunk {chunk}: first {live[0]}, middle {live[1]}, never {live[2]}, undecided {undecided}, "
          f"evaluated {int(consumed.sum())} of {C.MARCH_R * N}")
    assert undecided == 0
    assert live[0] > 0 and live[2] > 0 and (live[1] > 0 or len(range(chunk, N, chunk)) < 2)
