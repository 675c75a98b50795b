"""CPU-only checks of the hierarchical occupancy-grid build (avr.occupancy, csrc/occupancy_refine.hip, include/avr.h
"occupancy grid: hierarchical build"; additions within ABI 18): the five entries are exported and bound and refuse bad
arguments before any HIP call, the numpy reference of the GPU tests (tests/occupancy_refine_ref.py) holds the
contract's hand-made cases, the Python layer refuses what it must without a device, from_field(refine=None) is the
dense path, and the argument checks pass a host AddressSanitizer build driven by a stand-alone program. No kernel is
launched."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occupancy_ref as ref  # noqa: E402
import occupancy_refine_ref as rref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "adaptive-volume-rendering_amd")
ENTRIES = ("avr_occ_children", "avr_occ_child_points", "avr_occ_flag_sigma", "avr_occ_build_sparse",
           "avr_occ_downsample")
INVALID = 1001


def test_entries_are_exported_and_bound():
    from avr import _lib
    lib = _lib.load()
    assert lib.avr_version() == 18 == _lib.ABI_VERSION
    header = open(os.path.join(REPO, "include", "avr.h")).read()
    table = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert "occupancy grid: hierarchical build" in header
    for name in ENTRIES:
        assert name in _lib.EXPORTED and hasattr(lib, name) and re.search(rf"\bint {name}\(", header), name
        assert getattr(lib, name).argtypes == _lib._SIGS[name] and getattr(lib, name).restype is ctypes.c_int
        assert name in table, name
    for name in ("avr_occ_build", "avr_occ_scan", "avr_field_fwd_points"):     # the pieces the chain reuses stay
        assert name in _lib.EXPORTED and hasattr(lib, name)


def test_argument_checks_without_a_device():
    """Every refusal of include/avr.h through ctypes with null or host-only arguments: code 1001 and the stated
    message; n_live == 0 launches nothing and succeeds where the header says so."""
    from avr import _lib
    lib = _lib.load()
    host = (ctypes.c_double * 8)()
    hp = (ctypes.addressof(host) + 15) & ~15               # 16-B aligned; + 4: neither 8-B nor 16-B aligned
    odd = hp + 4
    err = lambda: lib.avr_last_error_string()  # noqa: E731
    I3, D3, F3 = ctypes.c_int * 3, ctypes.c_double * 3, ctypes.c_float * 3
    children, points, flag, sparse, down = (getattr(lib, n) for n in ENTRIES)

    def grid(res=(32, 8, 4), bits=hp):
        return ctypes.byref(_lib.OccGrid(F3(-1, -1, -1), F3(1, 1, 1), I3(*res), bits))

    res = I3(64, 16, 8)
    assert children(None, 2, res, hp, hp, None) == INVALID and b"null" in err()
    assert children(grid(bits=None), 2, res, hp, hp, None) == INVALID and b"null" in err()
    assert children(grid(), 2, None, hp, hp, None) == INVALID and b"null" in err()
    assert children(grid(), 2, res, None, hp, None) == INVALID and b"null" in err()
    assert children(grid(), 2, res, hp, None, None) == INVALID and b"null" in err()
    assert children(grid(), 2, res, odd, hp, None) == INVALID and b"aligned" in err()
    for f in (0, 1, 3, 5, 16, -2):
        assert children(grid(), f, res, hp, hp, None) == INVALID and b"factor" in err(), f
    assert children(grid(), 4, res, hp, hp, None) == INVALID and b"multiple of 32" in err()      # 64 / 4 = 16
    assert children(grid(), 2, I3(64, 15, 8), hp, hp, None) == INVALID and b"divisible" in err()
    assert children(grid((32, 8, 8)), 2, res, hp, hp, None) == INVALID and b"coarse res" in err()
    assert children(grid((40, 8, 4)), 2, res, hp, hp, None) == INVALID and b"multiple of 32" in err()
    assert children(grid(), 2, I3(288, 16, 8), hp, hp, None) == INVALID and b"res[0]" in err()

    lo, st, d = D3(-1, -1, -1), D3(0.1, 0.1, 0.1), F3(1, 0, 0)
    ok = [hp, hp, res, lo, st, d, 5, hp, hp, None]         # mask offsets res lo64 step dir n_live xyz viewdirs stream
    for i in (0, 1, 2, 3, 4):
        a = list(ok)
        a[i] = None
        assert points(*a) == INVALID and b"null" in err(), i
    a = list(ok)
    a[7] = a[8] = None
    assert points(*a) == INVALID and b"null" in err()
    a = list(ok)
    a[5] = None
    assert points(*a) == INVALID and b"null dir" in err()
    for i in (0, 1):
        a = list(ok)
        a[i] = odd
        assert points(*a) == INVALID and b"aligned" in err(), i
    for m in (-1, 64 * 16 * 8 + 1):
        a = list(ok)
        a[6] = m
        assert points(*a) == INVALID and b"n_live" in err(), m
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        a = list(ok)
        a[4] = D3(0.1, bad, 0.1)
        assert points(*a) == INVALID and b"step" in err(), bad
    a = list(ok)
    a[3] = D3(-1, float("nan"), -1)
    assert points(*a) == INVALID and b"lo64" in err()
    assert points(None, None, res, None, None, None, 0, None, None, None) == 0

    assert flag(None, 0.0, 1, 5, hp, None) == INVALID and b"null" in err()
    assert flag(hp, 0.0, 1, 5, None, None) == INVALID and b"null" in err()
    for thr in (-1e-6, -1.0, float("nan"), -float("inf")):
        assert flag(hp, thr, 1, 5, hp, None) == INVALID and b"thr" in err(), thr
    assert flag(hp, 0.0, 1, -1, hp, None) == INVALID and b"n_live" in err()
    assert flag(odd, 0.0, 1, 5, hp, None) == INVALID and b"aligned" in err()
    assert flag(None, 0.0, 1, 0, None, None) == 0

    ok = [hp, hp, hp, 5, res, 1, hp, None]                 # mask offsets flags n_live res dilate bits stream
    for i in (0, 1, 2, 4, 6):
        a = list(ok)
        a[i] = None
        assert sparse(*a) == INVALID and b"null" in err(), i
    assert sparse(None, None, None, 0, res, 1, None, None) == INVALID and b"null" in err()   # bits: always written
    for i, v, what in ((0, odd, b"aligned"), (1, odd, b"aligned"), (5, 3, b"dilate"), (5, -1, b"dilate"),
                       (3, -1, b"n_live"), (3, 64 * 16 * 8 + 1, b"n_live"), (4, I3(48, 16, 8), b"multiple of 32")):
        a = list(ok)
        a[i] = v
        assert sparse(*a) == INVALID and what in err(), (i, v)

    assert down(None, res, 2, hp, None) == INVALID and b"null" in err()
    assert down(hp, res, 2, None, None) == INVALID and b"null" in err()
    assert down(hp, None, 2, hp, None) == INVALID and b"null" in err()
    for p in (0, 3, 8, -1):
        assert down(hp, res, p, hp, None) == INVALID and b"not 1, 2 or 4" in err(), p
    assert down(hp, res, 4, hp, None) == INVALID and b"multiple of 32" in err()
    assert down(hp, I3(128, 16, 6), 4, hp, None) == INVALID and b"divisible" in err()
    assert not any(host)                                    # no refused or empty call wrote anything


# ------------------------------------------------------------------ the reference on hand-made cases
@pytest.mark.parametrize("f,rc", [(2, (32, 3, 2)), (4, (32, 2, 3)), (8, (32, 1, 2))])
def test_ref_candidate_order_and_ranks_for_a_single_live_coarse_cell(f, rc):
    res, _ = rref.check_shapes(tuple(r * f for r in rc), f)
    rx, ry, rz = res
    cases = {"corner": (0, 0, 0), "far corner": (rc[2] - 1, rc[1] - 1, rc[0] - 1), "face": (rc[2] - 1, 0, 17),
             "interior": (rc[2] // 2, rc[1] // 2, 20)}
    for name, (cz, cy, cx) in cases.items():
        cocc = np.zeros((rc[2], rc[1], rc[0]), bool)
        cocc[cz, cy, cx] = True
        cand = rref.children(cocc, f)
        mask, counts, offsets, M = rref.mask_counts_offsets(cand)
        assert M == f ** 3 == cand.sum() and mask.shape == (ry * rz, (rx + 63) // 64) and mask.dtype == np.uint64
        rows = [(cz * f + dz) * ry + cy * f + dy for dz in range(f) for dy in range(f)]       # ascending
        assert np.array_equal(np.nonzero(counts)[0], rows) and (counts[rows] == f).all(), name
        run = ((1 << f) - 1) << (cx * f % 64)                                                  # f cells in one word
        for j, row in enumerate(rows):
            assert offsets[row] == j * f and int(mask[row, cx * f // 64]) == run and int(mask[row].sum()) == run
        rk = rref.ranks(cand)
        lin = np.nonzero(cand.reshape(-1))[0]                                                  # ascending linear index
        assert np.array_equal(rk.reshape(-1)[lin], np.arange(M)) and (rk[~cand] == -1).all(), name
        first = (cz * f * ry + cy * f) * rx + cx * f
        assert lin[0] == first and lin[f] == first + rx                                       # x fastest, then y
        xyz, vd = rref.child_points(cand, (-1, -1, -1), (1, 1, 1), (0, 0, 1))
        cen = rref.centres((-1, -1, -1), (1, 1, 1), res).reshape(-1, 3)
        assert np.array_equal(xyz, cen[lin]) and (vd == np.float32([0, 0, 1])).all() and xyz.dtype == np.float32


def test_ref_ranks_across_mask_words_and_all_live():
    f, rc = 4, (64, 1, 2)                                         # rx = 256: four mask words per row
    cocc = np.zeros((2, 1, 64), bool)
    cocc[0, 0, [3, 15, 16, 40, 63]] = True                        # fine x 12..15 | 60..67 (crosses a word) | 160.. | 252..
    cocc[1] = True
    cand = rref.children(cocc, f)
    mask, counts, offsets, M = rref.mask_counts_offsets(cand)
    assert M == 4 ** 3 * cocc.sum() and counts[0] == 20 and counts[-1] == 256 and offsets[4] == 80
    assert int(mask[0, 0]) == (0xF << 12) | (0xF << 60) and int(mask[0, 1]) == 0xF
    assert int(mask[0, 2]) == 0xF << 32 and int(mask[0, 3]) == 0xF << 60 and int(mask[31, 2]) == 2 ** 64 - 1
    rk = rref.ranks(cand)
    assert rk[0, 0, 12] == 0 and rk[0, 0, 63] == 7 and rk[0, 0, 64] == 8 and rk[0, 0, 160] == 12 and rk[0, 0, 255] == 19
    assert rk[0, 1, 12] == 20 and rk[1, 0, 0] == -1 and rk[4, 0, 0] == 320 and rk[7, 3, 255] == M - 1
    # the centres are cell_centres' expression: float64 product and sum, each rounded once, then one float32 rounding
    lo, hi, res = (-0.45, -0.4, -0.35), (0.4, 0.45, 0.3), (256, 4, 8)
    lo64, step = rref.axes(lo, hi, res)
    assert lo64[0] == np.float64(np.float32(-0.45)) != -0.45 and step[0] == (np.float64(np.float32(0.4)) - lo64[0]) / 256
    c = rref.centres(lo, hi, res)
    assert c[5, 3, 77, 0] == np.float32(lo64[0] + 77.5 * step[0]) and c[5, 3, 77, 2] == np.float32(lo64[2] + 5.5 * step[2])
    from avr.occupancy import OccupancyGrid, refine_axes
    assert np.array_equal(c.reshape(-1, 3), OccupancyGrid.cell_centres(lo, hi, res, "cpu").numpy())
    own_lo, own_step = refine_axes(lo, hi, res)
    assert own_lo == list(lo64) and own_step == list(step)        # what the library is handed


@pytest.mark.parametrize("dilate", [0, 1, 2])
def test_ref_build_sparse_equals_dense_build_on_zero_filled_planes(dilate):
    rng = np.random.default_rng(21 + dilate)
    f, rc = 2, (32, 5, 4)
    cocc = rng.random((rc[2], rc[1], rc[0])) < 0.3
    cocc[0, 0, 0] = cocc[-1, -1, -1] = True                       # the two far corners: dilation meets the faces
    cocc[1, 1, 1] = False
    cand = rref.children(cocc, f)
    M = int(cand.sum())
    for K, thr in ((1, 0.0), (3, 0.0), (3, 0.4)):
        sigma = np.maximum(rng.standard_normal((K, M)) - 0.8, 0).astype(np.float32)       # ~ 20 % above zero
        sigma[rng.random((K, M)) < 0.01] = np.nan
        sigma[-1, 0], sigma[0, -1] = np.nan, 1.0
        flags = rref.flag_sigma(sigma, thr)
        assert flags.dtype == np.uint8 and set(np.unique(flags)) <= {0, 1} and flags[0] == 1 and flags[-1] == 1
        got = rref.build_sparse(cand, flags, dilate)
        want = ref.build(rref.dense_planes(cand, sigma), thr, dilate)
        assert np.array_equal(got, want) and got.any(), (K, thr)
        if dilate == 0:
            assert not got[~cand].any()                           # a cell under a dead parent is never set by itself
        else:
            assert got[~cand].any()                               # dilation crosses into dead parents
    at = np.full((1, M), 0.4, np.float32)                         # at the threshold is empty, above it occupied
    assert not rref.flag_sigma(at, 0.4).any() and rref.flag_sigma(at, 0.0).all()
    assert not rref.build_sparse(np.zeros_like(cand), np.zeros(0, np.uint8), dilate).any()    # M == 0


def test_ref_downsample_round_trip():
    rng = np.random.default_rng(4)
    for p, rc in ((1, (32, 3, 5)), (2, (32, 3, 5)), (4, (64, 2, 3))):
        cocc = rng.random((rc[2], rc[1], rc[0])) < 0.3
        fine = rref.children(cocc, p) if p > 1 else cocc.copy()
        assert np.array_equal(rref.downsample(fine, p), cocc)     # children, then the OR of the children
        one = np.zeros_like(fine)
        idx = tuple(int(v) for v in rng.integers(0, fine.shape))
        one[idx] = True                                           # one child is enough to set its parent
        d = rref.downsample(one, p)
        assert d.sum() == 1 and d[tuple(i // p for i in idx)]
        assert np.array_equal(ref.unpack_bits(ref.pack_bits(d), rc), d)


# ------------------------------------------------------------------ python layer without a device
def _grid(res=(32, 32, 32), lo=(-1, -1, -1), hi=(1, 1, 1)):
    from avr.occupancy import OccupancyGrid
    return OccupancyGrid.all_occupied(lo, hi, res, "cpu")


def test_refine_from_field_refusals(golden, monkeypatch):
    from helpers import build_net
    from avr import occupancy
    from avr.occupancy import OccupancyGrid
    net = build_net(golden("g4_field_small.npz"), "cpu")
    monkeypatch.setattr(occupancy, "children", lambda *a, **k: 1 / 0)          # no refusal may reach a launch
    coarse = _grid()
    with pytest.raises(ValueError, match="fused path"):
        OccupancyGrid.refine_from_field(torch.nn.Identity(), coarse, 2)
    for bad in (1, 3, 16, 0):
        with pytest.raises(ValueError, match="factor"):
            OccupancyGrid.refine_from_field(net, coarse, bad)
    with pytest.raises(ValueError, match="exceeds 256"):
        OccupancyGrid.refine_from_field(net, _grid((64, 32, 32)), 8)
    with pytest.raises(ValueError, match="box lo"):
        OccupancyGrid.refine_from_field(net, coarse, 2, lo=(-1, -1, -1.5), hi=(1, 1, 1))
    with pytest.raises(ValueError, match="box hi"):
        OccupancyGrid.refine_from_field(net, coarse, 2, lo=(-1, -1, -1), hi=(1, 1.25, 1))
    for bad in (-1e-9, -1.0, float("nan")):
        with pytest.raises(ValueError, match="sigma_thr"):
            OccupancyGrid.refine_from_field(net, coarse, 2, sigma_thr=bad)
    with pytest.raises(ValueError, match="dilate"):
        OccupancyGrid.refine_from_field(net, coarse, 2, dilate=3)
    # staleness: a keyed coarse grid must carry the net's current key; a grid without a key is accepted
    monkeypatch.setattr(occupancy, "field_key", lambda n: (("now",), []))
    coarse.key = ("then",)
    with pytest.raises(ValueError, match="have changed"):
        OccupancyGrid.refine_from_field(net, coarse, 2)
    for key in (("now",), None):
        coarse.key = key
        with pytest.raises(ZeroDivisionError):                                  # accepted: it reaches the chain
            OccupancyGrid.refine_from_field(net, coarse, 2, lo=(-1, -1, -1), hi=(1, 1, 1))
    # from_field(refine=...): the same, before any field evaluation
    monkeypatch.setattr(OccupancyGrid, "cell_centres", staticmethod(lambda *a, **k: 1 / 0))
    for kw, what in ((dict(refine=3), "refine"), (dict(refine=2, coarse_probe=3), "coarse_probe"),
                     (dict(refine=4, res=(64, 64, 64)), "multiple of 32"), (dict(refine=8, res=(256, 36, 64)), "divisible"),
                     (dict(refine=2, sigma_thr=-0.5), "sigma_thr")):
        kw.setdefault("res", (64, 64, 64))
        with pytest.raises(ValueError, match=what):
            OccupancyGrid.from_field(net, (-1,) * 3, (1,) * 3, **kw)
    with pytest.raises(ValueError, match="fused path"):
        OccupancyGrid.from_field(torch.nn.Identity(), (-1,) * 3, (1,) * 3, (64, 64, 64), refine=2)


def test_downsample_and_cells_missing_from_refusals():
    g = _grid((64, 32, 32))
    for p in (0, 3, 8, 4):                                       # 64 / 4 = 16: not a multiple of 32
        with pytest.raises(ValueError, match="downsample"):
            g.downsample(p)
    with pytest.raises(ValueError, match="downsample"):
        _grid((128, 32, 6)).downsample(4)
    with pytest.raises(Exception, match="HIP device"):
        g.downsample(2)                                          # valid, and there is no CPU path
    a, b = _grid(), _grid()
    assert a.cells_missing_from(b) == 0 and a.n_candidates is None and a.build_evals is None
    a.bits[5] = ~(1 << 7)
    a.bits[9] = 0
    assert a.cells_missing_from(b) == 33 and b.cells_missing_from(a) == 0
    for other in (_grid((64, 32, 32)), _grid(lo=(-1, -1, -2)), _grid(hi=(1, 2, 1))):
        with pytest.raises(ValueError, match="cells_missing_from"):
            a.cells_missing_from(other)


def test_from_field_without_refine_takes_the_dense_path(golden, monkeypatch):
    """refine=None (the default) never enters the hierarchical build: the dense planes go to from_sigma as before,
    with the arguments as before, and none of the new launches is made."""
    from helpers import build_net
    from avr import occupancy
    from avr.occupancy import OccupancyGrid
    net = build_net(golden("g4_field_small.npz"), "cpu")
    res, seen = (32, 4, 2), {}

    class Fused:
        def forward_points_scene(self, p, vd, coarse, sb):
            seen.setdefault("launches", []).append((p.shape[0], tuple(vd[0].tolist()), coarse, sb))
            return torch.cat([p, p[:, :1] * 0 + len(seen["launches"])], 1)

    def from_sigma(planes, lo, hi, thr, dilate=1, key=None, keep=None):
        seen["sigma"] = (planes.clone(), lo, hi, thr, dilate, key)
        return OccupancyGrid.all_occupied(lo, hi, res, "cpu")

    monkeypatch.setattr(net, "fused", lambda: Fused(), raising=False)
    monkeypatch.setattr(occupancy, "field_key", lambda n: (("k",), []))
    monkeypatch.setattr(OccupancyGrid, "from_sigma", staticmethod(from_sigma))
    for name in ("refine_from_field", "_from_field_refined", "downsample"):
        monkeypatch.setattr(OccupancyGrid, name, lambda *a, **k: 1 / 0)
    for name in ("children", "child_points", "flag_sigma", "build_sparse"):
        monkeypatch.setattr(occupancy, name, lambda *a, **k: 1 / 0)
    for kw in ({}, {"refine": None, "coarse_dilate": 2, "coarse_probe": 4}):   # the knobs mean nothing without refine
        seen.clear()
        g = OccupancyGrid.from_field(net, (-1, -1, -1), (1, 1, 1), res, sigma_thr=0.25, dilate=2, chunk=100, **kw)
        n = 32 * 4 * 2
        planes, lo, hi, thr, dilate, key = seen["sigma"]
        assert planes.shape == (12, 2, 4, 32) and (thr, dilate, key) == (0.25, 2, ("k",)) and lo == (-1, -1, -1)
        assert [l[0] for l in seen["launches"]] == [100, 100, 56] * 12                 # chunks of every plane
        assert [l[2] for l in seen["launches"][::3]] == [True] * 6 + [False] * 6
        assert [l[1] for l in seen["launches"][::3]] == list(occupancy.AXIS_DIRS) * 2
        assert planes[0].reshape(-1)[0] == 1 and planes[11].reshape(-1)[-1] == 36      # each launch's channel 3
        assert g.build_evals == 12 * n and g.n_candidates is None


def test_cli_and_render_orbit_refine_arguments(capsys):
    from avr import render
    from avr.video import render_orbit
    for argv, what in ((["--occupancy-refine", "2"], "--occupancy-refine needs --occupancy"),
                       (["--occupancy", "64", "--occupancy-probe", "2"], "--occupancy-probe needs --occupancy-refine"),
                       (["--occupancy", "64", "--occupancy-refine", "3"], "--occupancy-refine must be one of"),
                       (["--occupancy", "64", "--occupancy-refine", "2", "--occupancy-probe", "3"],
                        "--occupancy-probe must be one of"),
                       (["--occupancy", "64", "--occupancy-refine", "4"], "a multiple of 128")):
        with pytest.raises(SystemExit) as e:
            render.main(argv)
        assert e.value.code == 2 and what in capsys.readouterr().err, argv
    with pytest.raises(ValueError, match="occupancy_refine needs occupancy"):
        render_orbit(None, None, torch.eye(3), 1, 1.0, 8, occupancy_refine=2)
    with pytest.raises(ValueError, match="occupancy_probe needs occupancy_refine"):
        render_orbit(None, None, torch.eye(3), 1, 1.0, 8, occupancy=64, occupancy_probe=2)
    with pytest.raises(ValueError, match="occupancy_refine must be one of"):
        render_orbit(None, None, torch.eye(3), 1, 1.0, 8, occupancy=64, occupancy_refine=5)


def test_occupancy_refine_abi_check_under_host_asan():
    """tests/occupancy_refine_abi_check.c against the host-AddressSanitizer build of the library
    (`make asan-occupancy-refine`), run as a program of its own: nothing is preloaded and nothing is loaded into
    Python."""
    b = subprocess.run(["make", "-C", PKG, "asan-occupancy-refine", "-j8"], capture_output=True, text=True,
                       timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([os.path.join(PKG, "build", "occupancy_refine_abi_check_asan")], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "occupancy_refine_abi_check: 0 failure(s)" in r.stdout
    assert "AddressSanitizer" not in r.stderr
