"""The hierarchical occupancy-grid build (avr.occupancy, csrc/occupancy_refine.hip; not in the reference) on the
device: the five kernels against the numpy restatement of the contract (tests/occupancy_refine_ref.py) bit for bit,
refine_from_field against the test's own enumeration and evaluation of the candidates, against the dense build on
zero-filled planes, and from_field(refine=...) against its three steps made by hand, a render and the CLI.

Shapes (fine res, factor -> coarse res): (64, 16, 16) / 2 -> (32, 8, 8), one mask word per row; (128, 8, 12) / 4 ->
(32, 2, 3), two words; (256, 8, 8) / 8 -> (32, 1, 1), four words. The box is that of tests/test_gpu_occupancy.py.
Everything but the rendered image is held to bit equality: the chain has no arithmetic beyond the double centres and
the comparisons, and the x3 field (whose rows depend on which 64 rows share a workgroup) is evaluated by the test in
the build's own chunks.

The fixture nets are random fog, nearly all-occupied as they are; lin_out.bias[3] of both MLPs is shifted so that the
coarse grid of a field test has dead and live parents, and every such test asserts a live share in [0.1, 0.9]."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occupancy_ref as ref  # noqa: E402
import occupancy_refine_ref as rref  # noqa: E402
from helpers import build_net, to_np  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
LO, HI = (-0.45, -0.4, -0.35), (0.4, 0.45, 0.3)
CENTRE, RADIUS = (0.02, -0.03, 0.05), 0.3
SHAPES = {"one-word": ((64, 16, 16), 2), "two-words": ((128, 8, 12), 4), "four-words": ((256, 8, 8), 8)}
# fixture, shift of lin_out.bias[3], coarse_dilate: the combinations whose coarse live share at (64, 16, 16) / 2 lies
# well inside [0.1, 0.9] (0.318, 0.794, 0.313, 0.550 with the CPU oracle)
FOG = [("g4_field_small", -0.5, 0), ("g4_field_small", -0.5, 1), ("g4_field_full", -2.0, 0), ("g4_field_full", -4.0, 1)]
CHUNK = 2048
_NETS = {}


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _net(golden, fixture, shift, precision):
    key = (fixture, shift, precision)
    if key not in _NETS:
        net = build_net(golden(fixture + ".npz"), DEV, precision)
        with torch.no_grad():                                   # before the net's first use: nothing is cached yet
            for mlp in (net.mlp_coarse, net.mlp_fine):
                mlp.lin_out.bias[3] += shift
        _NETS[key] = net
    return _NETS[key]


def _bits(grid):
    return grid.bits.cpu().numpy().view(np.uint32)


def _grid(occ, res, lo=LO, hi=HI):
    from avr.occupancy import OccupancyGrid
    return OccupancyGrid(lo, hi, res, T(ref.pack_bits(occ).view(np.int32)))


def _coarse_occ(kind, rc):
    rx, ry, rz = rc
    if kind == "sphere":
        return ref.sphere_occ(rc, LO, HI, CENTRE, RADIUS)
    if kind == "corner":
        occ = np.zeros((rz, ry, rx), bool)
        occ[-1, -1, -1] = True
        return occ
    if kind == "mixed":                                          # live and dead parents next to each other, both
        occ = np.random.default_rng(5).random((rz, ry, rx)) < 0.4   # far corners live so dilation meets the faces
        occ[0, 0, 0] = occ[-1, -1, -1] = True
        occ[0, 0, 1] = False
        return occ
    return np.full((rz, ry, rx), kind == "all")


def _chain(coarse, f, res, direction=(0.0, -1.0, 0.0)):
    from avr import occupancy
    mask, counts = occupancy.children(coarse, f, res)
    offsets, total = occupancy.scan(counts)
    M = int(total.item())
    xyz = vd = None
    if M:
        xyz, vd = occupancy.child_points(mask, offsets, res, LO, HI, M, direction)
    return mask, counts, offsets, M, xyz, vd


# ------------------------------------------------------------------ 1. children / scan / child_points
@pytest.mark.parametrize("kind", ["sphere", "all", "none", "corner"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_children_scan_points_match_reference(shape, kind):
    from avr.occupancy import OccupancyGrid
    res, f = SHAPES[shape]
    res, rc = rref.check_shapes(res, f)
    cocc = _coarse_occ(kind, rc)
    cand = rref.children(cocc, f)
    mask_r, counts_r, offsets_r, M_r = rref.mask_counts_offsets(cand)
    assert M_r == f ** 3 * int(cocc.sum())
    coarse = _grid(cocc, rc)
    direction = (0.0, -1.0, 0.0)
    runs = []
    for _ in range(2):
        mask, counts, offsets, M, xyz, vd = _chain(coarse, f, res, direction)
        torch.cuda.synchronize()
        runs.append([t.cpu().numpy() for t in (mask, counts, offsets)] + ([xyz.cpu().numpy(), vd.cpu().numpy()] if M else []))
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))                    # two runs are bit-equal
    assert M == M_r and (kind != "sphere" or 0 < M < cand.size)
    assert np.array_equal(runs[0][0].view(np.uint64), mask_r) and np.array_equal(runs[0][1], counts_r)
    assert np.array_equal(runs[0][2], offsets_r)
    if not M:
        assert kind == "none"
        return
    xyz_r, vd_r = rref.child_points(cand, LO, HI, direction)
    assert np.array_equal(runs[0][3].view(np.uint32), xyz_r.view(np.uint32))
    assert np.array_equal(runs[0][4].view(np.uint32), vd_r.view(np.uint32))          # (-0.0 stays -0.0)
    centres = to_np(OccupancyGrid.cell_centres(LO, HI, res, DEV))
    assert np.array_equal(runs[0][3], centres[cand.reshape(-1)])
    if kind == "all":
        assert np.array_equal(runs[0][3], centres)
    # one output left out: the other is written alike, and the one kept from before is not touched
    from avr import occupancy
    keep = torch.full_like(xyz, 7.0)
    _, vd2 = occupancy.child_points(mask, offsets, res, LO, HI, M, (0.5, 0.25, -1.0), xyz=False, viewdirs=keep)
    xyz2, none = occupancy.child_points(mask, offsets, res, LO, HI, M, direction, viewdirs=False)
    assert vd2 is keep and none is None and np.array_equal(to_np(xyz2), xyz_r)
    assert (to_np(vd2) == np.float32([0.5, 0.25, -1.0])).all()


# ------------------------------------------------------------------ 2. flag_sigma / build_sparse
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_flag_sigma_and_build_sparse_match_reference(shape):
    from avr import occupancy
    res, f = SHAPES[shape]
    res, rc = rref.check_shapes(res, f)
    cocc = _coarse_occ("mixed", rc)
    cand = rref.children(cocc, f)
    mask, counts, offsets, M, _, _ = _chain(_grid(cocc, rc), f, res)
    assert M == int(cand.sum()) and 0 < M < cand.size
    rng = np.random.default_rng(13)
    for K in (1, 3):
        field = rng.random((K, M, 4)).astype(np.float32)
        sigma = np.maximum(rng.standard_normal((K, M)) - 1.2, 0).astype(np.float32)   # ~ 12 % above zero per plane
        sigma[rng.random((K, M)) < 2e-3] = np.nan
        sigma[0, 0], sigma[-1, -1] = 1.0, np.nan                                        # the first and last candidate
        field[..., 3] = sigma
        for thr in (0.0, 0.4):
            flags = torch.full((M,), 255, dtype=torch.uint8, device=DEV)                # plane 0 must overwrite
            for k in range(K):
                occupancy.flag_sigma(T(field[k]), thr, k == 0, flags)
            flags_r = rref.flag_sigma(sigma, thr)
            assert np.array_equal(flags.cpu().numpy(), flags_r), (K, thr)
            dense = rref.dense_planes(cand, sigma)
            for dilate in (0, 1, 2):
                bits = occupancy.build_sparse(mask, offsets, flags, M, res, dilate)
                want = rref.build_sparse(cand, flags_r, dilate)
                got = ref.unpack_bits(bits.cpu().numpy(), res)
                assert np.array_equal(got, want), (K, thr, dilate)
                assert np.array_equal(want, ref.build(dense, thr, dilate))              # the dense build's bits
                assert got.any() and (dilate == 0) == (not got[~cand].any())           # dilation crosses to dead parents
                assert got[0, 0, 0] and got[-1, -1, -1]                                 # and meets the faces
    # M == 0: every word is written, with zeros, and nothing else is read
    none = _grid(_coarse_occ("none", rc), rc)
    mask0, counts0, offsets0, M0, _, _ = _chain(none, f, res)
    bits0 = occupancy.build_sparse(mask0, offsets0, None, M0, res, 2)
    assert M0 == 0 and not bits0.cpu().numpy().any() and not counts0.cpu().numpy().any()


def test_downsample_matches_reference():
    rng = np.random.default_rng(8)
    for res, p in (((64, 16, 16), 1), ((64, 16, 16), 2), ((128, 8, 12), 4), ((256, 6, 4), 2)):
        occ = rng.random((res[2], res[1], res[0])) < 0.01
        occ[-1, -1, -1] = True
        g = _grid(occ, res)
        g.key = ("k",)
        d = g.downsample(p)
        want = rref.downsample(occ, p)
        assert d.res == tuple(r // p for r in res) and d.lo == g.lo and d.hi == g.hi and d.key == ("k",)
        assert np.array_equal(ref.unpack_bits(_bits(d), d.res), want) and 0 < want.mean() < 1
        assert d.bits.data_ptr() != g.bits.data_ptr()
        back = rref.children(want, p) if p > 1 else want         # every child of a set parent: a superset of occ
        up = _grid(back, res)
        assert up.cells_missing_from(g) == 0 and g.cells_missing_from(up) == int((back & ~occ).sum())


# ------------------------------------------------------------------ 3. refine_from_field, the test's own evaluation
def _own_candidates(coarse, f):
    """The candidates from the coarse grid's bits, on the host: cand (rz, ry, rx) and their centres (M, 3)."""
    cocc = ref.unpack_bits(_bits(coarse), coarse.res)
    cand = rref.children(cocc, f)
    res = tuple(r * f for r in coarse.res)
    return cocc, cand, rref.centres(coarse.lo, coarse.hi, res)[cand]


def _own_sigma(net, xyz, chunk):
    """sigma of both MLPs for the six axis directions at xyz (M, 3) through fused.forward_points in chunks of
    `chunk` rows: (12, M)."""
    from avr.occupancy import AXIS_DIRS
    fused, pts, planes = net.fused(), T(xyz), []
    with torch.no_grad():
        for coarse in (True, False):
            for d in AXIS_DIRS:
                vd = torch.tensor([d], device=DEV)
                parts = [fused.forward_points(pts[c0:c0 + chunk][None],
                                              vd.expand(min(chunk, len(pts) - c0), 3)[None], coarse)[0, :, 3]
                         for c0 in range(0, len(pts), chunk)]
                planes.append(torch.cat(parts))
    return to_np(torch.stack(planes))


def _fog_coarse(net, rc, coarse_dilate):
    from avr.occupancy import OccupancyGrid
    coarse = OccupancyGrid.from_field(net, LO, HI, rc, sigma_thr=0.0, dilate=coarse_dilate, chunk=CHUNK)
    share = coarse.live_fraction()
    print(f"coarse {rc} dilate {coarse_dilate}: live share {share:.3f}")
    assert 0.1 <= share <= 0.9, share                            # dead and live parents both occur
    return coarse


# the four combinations at the first shape, and the first of them at the other two (shares 0.396 and 0.281 there)
FOG_CASES = [("one-word",) + c for c in FOG] + [(s,) + FOG[0] for s in ("two-words", "four-words")]


@pytest.mark.parametrize("precision", ["fp32", "x3"])
@pytest.mark.parametrize("shape,fixture,shift,coarse_dilate", FOG_CASES)
def test_refine_from_field_equals_own_evaluation_of_the_candidates(golden, shape, fixture, shift, coarse_dilate,
                                                                   precision):
    from avr.occupancy import OccupancyGrid
    net = _net(golden, fixture, shift, precision)
    res, f = SHAPES[shape]
    coarse = _fog_coarse(net, tuple(r // f for r in res), coarse_dilate)
    cocc, cand, xyz = _own_candidates(coarse, f)
    M = int(cand.sum())
    sigma = _own_sigma(net, xyz, CHUNK)
    assert M > CHUNK                                             # several chunks: the x3 grouping matters
    for thr, dilate in ((0.0, 1), (0.0, 0), (0.05, 2)):
        grid = OccupancyGrid.refine_from_field(net, coarse, f, sigma_thr=thr, dilate=dilate, chunk=CHUNK)
        want = rref.build_sparse(cand, rref.flag_sigma(sigma, thr), dilate)
        assert grid.res == res and grid.lo == coarse.lo and grid.hi == coarse.hi
        assert np.array_equal(ref.unpack_bits(_bits(grid), res), want), (thr, dilate)
        assert grid.n_candidates == M == f ** 3 * int(cocc.sum()) and grid.build_evals == 12 * M
        assert grid.key is not None and not grid.stale(net)
    print(f"{fixture} {shift} {precision}: M = {M} of {cand.size}, fine live share {want.mean():.3f}")


# ------------------------------------------------------------------ 4. fp32: the dense build on zero-filled planes
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fp32_refine_equals_dense_build_with_non_candidates_zeroed(golden, shape):
    from avr.occupancy import OccupancyGrid
    net = _net(golden, "g4_field_small", -0.5, "fp32")
    res, f = SHAPES[shape]
    res, rc = rref.check_shapes(res, f)
    # (the sphere grid: its share does not depend on the field; the fog's own coarse grid is case 3's and 5's)
    cocc = _coarse_occ("sphere", rc)
    assert 0.1 <= cocc.mean() <= 0.9
    cand = rref.children(cocc, f)
    centres = rref.centres(LO, HI, res).reshape(-1, 3)
    dense = _own_sigma(net, centres, 8192).reshape(12, res[2], res[1], res[0])       # as the dense build evaluates
    assert (dense[:, ~cand] > 0).any()                             # zeroing the non-candidates changes something
    dense[:, ~cand] = 0
    for dilate in (0, 1, 2):
        grid = OccupancyGrid.refine_from_field(net, _grid(cocc, rc), f, sigma_thr=0.0, dilate=dilate, chunk=CHUNK)
        assert np.array_equal(ref.unpack_bits(_bits(grid), res), ref.build(dense, 0.0, dilate)), dilate
    # an all-live coarse grid: the dense from_field, bit for bit
    full = OccupancyGrid.refine_from_field(net, OccupancyGrid.all_occupied(LO, HI, rc, DEV), f, chunk=CHUNK)
    dense_grid = OccupancyGrid.from_field(net, LO, HI, res, chunk=8192)
    assert np.array_equal(_bits(full), _bits(dense_grid)) and full.n_candidates == cand.size
    assert full.build_evals == dense_grid.build_evals == 12 * cand.size and dense_grid.n_candidates is None
    assert full.cells_missing_from(dense_grid) == 0
    print(f"{shape}: the sphere-refined grid lacks {grid.cells_missing_from(dense_grid)} of the dense grid's cells")


def test_empty_coarse_grid_gives_zero_bits_and_launches_no_field(golden, monkeypatch):
    from avr.occupancy import OccupancyGrid
    net = _net(golden, "g4_field_small", -0.5, "fp32")
    res, f = SHAPES["two-words"]
    rc = tuple(r // f for r in res)
    fused = net.fused()
    calls = []
    monkeypatch.setattr(fused, "forward_points_scene", lambda *a, **k: calls.append(a) or 1 / 0)
    grid = OccupancyGrid.refine_from_field(net, _grid(_coarse_occ("none", rc), rc), f, dilate=2)
    torch.cuda.synchronize()
    assert not calls and not _bits(grid).any() and grid.n_candidates == 0 and grid.build_evals == 0
    assert grid.res == res and grid.live_fraction() == 0.0


# ------------------------------------------------------------------ 5. from_field(refine=...), staleness, a render
@pytest.mark.parametrize("probe", [1, 2])
@pytest.mark.parametrize("fixture,shift,coarse_dilate", [FOG[0], FOG[3]])
def test_from_field_refine_equals_its_three_steps(golden, fixture, shift, coarse_dilate, probe):
    from avr.occupancy import OccupancyGrid
    net = _net(golden, fixture, shift, "x3")
    res, f = SHAPES["one-word"]
    rc = tuple(r // f for r in res)
    grid = OccupancyGrid.from_field(net, LO, HI, res, sigma_thr=0.0, dilate=1, chunk=CHUNK, refine=f,
                                    coarse_dilate=coarse_dilate, coarse_probe=probe)
    by_hand = OccupancyGrid.from_field(net, LO, HI, tuple(r * probe for r in rc), sigma_thr=0.0, dilate=coarse_dilate,
                                       chunk=CHUNK)
    coarse = by_hand.downsample(probe)
    share = coarse.live_fraction()
    print(f"{fixture} {shift} probe {probe}: coarse live share {share:.3f}")
    assert 0.1 <= share <= 0.9, share                            # (CPU oracle: 0.318 / 0.572 and 0.550 / 0.708)
    own = OccupancyGrid.refine_from_field(net, coarse, f, sigma_thr=0.0, dilate=1, chunk=CHUNK)
    assert np.array_equal(_bits(grid), _bits(own)) and grid.res == res and grid.lo == own.lo and grid.hi == own.hi
    M = f ** 3 * int(ref.unpack_bits(_bits(coarse), rc).sum())
    probe_cells = rc[0] * rc[1] * rc[2] * probe ** 3
    assert grid.n_candidates == own.n_candidates == M and grid.build_evals == 12 * (probe_cells + M)
    assert grid.key == own.key and not grid.stale(net)
    if probe == 1:                                               # p = 1: downsample is a copy of the probe's bits
        assert np.array_equal(_bits(coarse), _bits(by_hand))


def test_refined_grid_goes_stale_and_renders_like_the_masked_chain(golden):
    import test_gpu_occupancy as base
    from avr.cache import bump_param_generation
    from avr.occupancy import OccupancyGrid
    net = build_net(golden("g4_field_full.npz"), DEV, "x3")       # its own net: a parameter is changed below
    with torch.no_grad():
        for mlp in (net.mlp_coarse, net.mlp_fine):
            mlp.lin_out.bias[3] += -2.0
    res, f = SHAPES["one-word"]
    grid = OccupancyGrid.from_field(net, LO, HI, res, refine=f, coarse_dilate=0, chunk=CHUNK)
    coarse = OccupancyGrid.from_field(net, LO, HI, tuple(r // f for r in res), dilate=0, chunk=CHUNK)
    assert 0.1 <= coarse.live_fraction() <= 0.9 and 0 < grid.live_fraction() < 1
    R = 1024
    x_pix, c2w, K = base._camera(R)
    occ = ref.unpack_bits(_bits(grid), res)
    w_c, w_f, w_d, (n_c, n_f) = base._masked_chain(net, x_pix, c2w, K, occ)
    g_c, g_f, g_d, rend = base._render(net, x_pix, c2w, K, grid)
    base._compare("x3", (g_c, g_f, g_d), (w_c, w_f, w_d), "refined grid vs masked chain")
    assert rend.last_live_by_pass[0] == n_c and 0 < n_c < R * 128
    with torch.no_grad():
        net.mlp_fine.lin_out.bias[3] += 0.25                     # changed in place ...
    bump_param_generation()                                      # ... and announced
    assert grid.stale(net) and coarse.stale(net)
    with pytest.raises(ValueError, match="have changed"):
        base._render(net, x_pix, c2w, K, grid)
    with pytest.raises(ValueError, match="have changed"):
        OccupancyGrid.refine_from_field(net, coarse, f)
    coarse.key = None                                            # a grid no net's state can make stale is accepted
    again = OccupancyGrid.refine_from_field(net, coarse, f, chunk=CHUNK)
    assert not again.stale(net) and again.n_candidates == grid.n_candidates


# ------------------------------------------------------------------ 6. the CLI
def test_cli_occupancy_refine_end_to_end(capsys):
    from avr import render
    render.main(["--frames", "1", "--res", "32", "--warmup", "0", "--occupancy", "64", "--occupancy-refine", "2"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["occupancy"] == 64 and line["occupancy_refine"] == 2 and line["occupancy_build_ms"] > 0
    evals = line["occupancy_build_evals"]
    assert evals % 12 == 0 and evals // 12 >= 32 ** 3 and (evals // 12 - 32 ** 3) % 8 == 0   # 12 (32^3 + 8 live)
    assert evals // 12 <= 32 ** 3 + 64 ** 3 and 0 <= line["occupancy_cells_set"] <= 1
    assert 0 <= line["live_samples_fraction"] <= 1
    dense = ["--frames", "1", "--res", "32", "--warmup", "0", "--occupancy", "64"]
    render.main(dense)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["occupancy_refine"] is None and line["occupancy_build_evals"] == 12 * 64 ** 3
