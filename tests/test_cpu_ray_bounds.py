"""CPU-only checks of the per-ray sampling bounds (avr_occ_ray_bounds, avr_sample_coarse_bounds,
avr_sample_fine_bounds; include/avr.h "occupancy grid: per-ray bounds", additions within ABI 18): the three entries are
exported and bound, the numpy reference of the GPU tests (tests/ray_bounds_ref.py) is anchored to the live test of
tests/occupancy_ref.py, at most 10 % of every ray set the GPU tests use is in between a clear hit and a clear miss,
the Python layer refuses what it must without a device, and the argument checks pass a host AddressSanitizer build
driven by a stand-alone program. No kernel is launched."""
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
import ray_bounds_ref as rb  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "adaptive-volume-rendering_amd")
ENTRIES = ("avr_occ_ray_bounds", "avr_sample_coarse_bounds", "avr_sample_fine_bounds")
F = np.float32


def test_entries_are_exported_and_bound():
    from avr import _lib
    lib = _lib.load()
    assert lib.avr_version() == 18 == _lib.ABI_VERSION
    header = open(os.path.join(REPO, "include", "avr.h")).read()
    table = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert "occupancy grid: per-ray bounds" in header
    for name in ENTRIES:
        assert name in _lib.EXPORTED and hasattr(lib, name) and re.search(rf"\bint {name}\(", header), name
        assert getattr(lib, name).argtypes == _lib._SIGS[name] and getattr(lib, name).restype is ctypes.c_int
        assert name in table, name
    # the per-ray forms take the scalar entries' parameters with two pointers for the two floats
    assert len(_lib._SIGS["avr_sample_coarse_bounds"]) == len(_lib._SIGS["avr_sample_coarse"])
    assert len(_lib._SIGS["avr_sample_fine_bounds"]) == len(_lib._SIGS["avr_sample_fine"])


@pytest.mark.parametrize("radius", [0.5, 0.35])
def test_reference_hull_holds_every_live_sample(radius):
    """The float64 hull and the two classes against the fp32 live test: on the 16 x 16 fan over the 32^3 sphere
    grid with 4 096 depths per ray, every depth occupancy_ref.classify calls live lies in the hull widened by the
    slack, and a clear miss has no live depth."""
    occ = rb.sphere_grid(radius)
    ro, rd = rb.fan()
    clear_hit, clear_miss, a, b = rb.classes(occ, rb.LO, rb.HI, ro, rd, rb.NEAR, rb.FAR)
    assert clear_hit.sum() >= 40 and clear_miss.sum() >= 100           # both classes are well filled
    z = rb.dense_z(rb.NEAR, rb.FAR, len(ro), 4096)
    live, _, _ = ref.classify(occ, rb.LO, rb.HI, ro, rd, z)
    assert live.any(1)[clear_hit].all()                                # a clear hit crosses a cell for > 0.75 of it
    assert not live[clear_miss].any()
    s = rb.slack(rd, rb.LO, rb.HI, rb.RES)
    assert rb.live_outside(live, z.astype(np.float64), a - s, b + s) == 0
    # and the hull is no wider than the live depths need: within two sample spacings plus the slack of them
    has = live.any(1)
    first = np.where(live, z, np.inf).min(1)[has]
    last = np.where(live, z, -np.inf).max(1)[has]
    dz = (rb.FAR - rb.NEAR) / 4095
    assert (first - a[has] <= s[has] + 2 * dz).all() and (b[has] - last <= s[has] + 2 * dz).all()


def test_reference_hull_by_hand():
    """One occupied cell, rays along an axis: the hull is the cell's extent along the ray, clipped."""
    occ = np.zeros((32, 32, 32), bool)
    occ[16, 16, 16] = True                                             # [0, 0.0625]^3
    ro = np.array([[0.03, 0.03, -1.0], [0.03, 0.03, -1.0], [0.5, 0.03, -1.0], [0.0701, 0.03, -1.0]], F)
    rd = np.array([[0, 0, 1.0], [0, 0, 2.0], [0, 0, 1.0], [0, 0, 1.0]], F)
    hit, a, b = rb.hull(occ, rb.LO, rb.HI, ro, rd, 0.1, 1.05)
    assert hit.tolist() == [True, True, False, False]
    assert np.allclose(a[:2], [1.0, 0.5]) and np.allclose(b[:2], [1.05, 0.53125])      # far cuts the first
    assert (a[2:] == float(F(0.1))).all() and (b[2:] == float(F(1.05))).all()       # the entry's two floats
    ch, cm, _, _ = rb.classes(occ, rb.LO, rb.HI, ro, rd, 0.1, 1.05)
    assert ch.tolist() == [True, True, False, False]
    assert cm.tolist() == [False, False, True, False]                  # the last passes 0.0076 beside: in between
    assert np.allclose(rb.slack(rd, rb.LO, rb.HI, rb.RES), np.sqrt(3) * 0.0625 / np.array([1, 2, 1, 1]))


def test_in_between_share_of_every_gpu_ray_set():
    """At most 10 % of every ray set tests/test_gpu_ray_bounds.py runs is neither a clear hit nor a clear miss; the
    24 x 24 fan and the smaller sphere, which it does not run, stay below it too."""
    for name, c in rb.cases().items():
        share = rb.in_between_share(c["occ"], c["lo"], c["hi"], c["ro"], c["rd"], c["near"], c["far"])
        assert share <= 0.10, (name, share)
    ch, cm, _, _ = rb.classes(*[rb.cases()["sphere_fan_256"][k] for k in ("occ", "lo", "hi", "ro", "rd", "near", "far")])
    assert ch.sum() > 64 and cm.sum() > 64
    assert rb.in_between_share(rb.sphere_grid(), rb.LO, rb.HI, *rb.fan(24), rb.NEAR, rb.FAR) <= 0.10
    assert rb.in_between_share(rb.sphere_grid(0.35), rb.LO, rb.HI, *rb.fan(), rb.NEAR, rb.FAR) <= 0.10
    # the cases hold what they are named for
    c = rb.cases()
    assert (c["axis_parallel"]["rd"] == 0).any(1).all()
    assert not np.isfinite(c["non_finite"]["rd"]).all() and not np.isfinite(c["non_finite"]["ro"]).all()
    _, _, a, b = rb.classes(*[c["far_cut"][k] for k in ("occ", "lo", "hi", "ro", "rd", "near", "far")])
    assert (b == F(1.3)).sum() > 32                                    # far cuts these hulls
    lo, hi = np.asarray(rb.LO), np.asarray(rb.HI)
    assert ((c["inside_box"]["ro"] > lo) & (c["inside_box"]["ro"] < hi)).all()
    seg = c["full"]["ro"][:, None] + c["full"]["rd"][:, None] * np.array([rb.NEAR, rb.FAR])[None, :, None]
    assert ((seg > lo) & (seg < hi)).all()                             # the box holds every [near, far] segment


def _grid():
    from avr.occupancy import OccupancyGrid
    return OccupancyGrid.all_occupied((-1, -1, -1), (1, 1, 1), (32, 32, 32), "cpu")


def test_check_skip_modes_ray_bounds_keyword():
    from avr.renderers import check_skip_modes
    g = _grid()
    for occ, count in ((None, "host"), (g, "host"), (g, "device")):    # the default changes no answer
        check_skip_modes("x: ", None, "host", occ, count)
        check_skip_modes("x: ", None, "host", occ, count, ray_bounds=None)
    check_skip_modes("x: ", None, "host", g, "host", ray_bounds="grid")
    check_skip_modes("x: ", 1e-3, "device", g, "device", capture=True, ray_bounds="grid")
    with pytest.raises(ValueError, match="needs occupancy"):
        check_skip_modes("x: ", None, "host", None, "host", ray_bounds="grid")
    with pytest.raises(ValueError, match="--ray-bounds needs --occupancy"):
        check_skip_modes("", None, None, None, None, idle=None, name=lambda n: "--" + n.replace("_", "-"),
                         ray_bounds="grid")
    for bad in ("cells", True, 0, "Grid"):
        with pytest.raises(ValueError, match="must be None or 'grid'"):
            check_skip_modes("x: ", None, "host", g, "host", ray_bounds=bad)
    with pytest.raises(ValueError, match="cannot be captured"):         # the other rules still hold with it
        check_skip_modes("x: ", None, "host", g, "host", capture=True, ray_bounds="grid")


def _call(rend, grad=False, net=None):
    R = 8
    args = (torch.eye(4).reshape(1, 1, 4, 4).expand(1, R, 4, 4), torch.eye(3)[None], torch.rand(1, R, 2))
    with torch.set_grad_enabled(grad):
        return rend(*args, net if net is not None else torch.nn.Identity())


def test_renderer_refusals_without_a_device():
    """ValueError, never a quiet render without bounds: without occupancy, under autograd, on the module path, for
    another value; render_orbit and GraphedRenderer refuse the same."""
    from avr.graphs import GraphedRenderer
    from avr.renderers import VolumeRenderer
    from avr.video import render_orbit
    rend = VolumeRenderer(0.8, 1.8, 32, 16, 0, 0.01, True)
    assert rend.ray_bounds is None and rend.last_ray_bounds is None
    for bad in ("cells", 1, "GRID"):
        with pytest.raises(ValueError, match="must be None or 'grid'"):
            rend.ray_bounds = bad
    assert rend.ray_bounds is None
    rend.ray_bounds = "grid"
    with pytest.raises(ValueError, match="needs occupancy"):            # no grid
        _call(rend)
    with pytest.raises(ValueError, match="needs occupancy"):
        _call(rend, grad=True)
    rend.occupancy = _grid()
    with pytest.raises(ValueError, match="inference only"):             # autograd
        _call(rend, grad=True)
    with pytest.raises(ValueError, match="fused path"):                 # the module path
        _call(rend)
    with pytest.raises(ValueError, match="cannot be captured"):         # host count in a graph
        GraphedRenderer(rend, torch.nn.Identity(), torch.eye(4).reshape(1, 1, 4, 4), torch.eye(3)[None],
                        torch.rand(1, 8, 2))
    rend.occupancy = None
    with pytest.raises(ValueError, match="needs renderer.occupancy"):
        GraphedRenderer(rend, torch.nn.Identity(), torch.eye(4).reshape(1, 1, 4, 4), torch.eye(3)[None],
                        torch.rand(1, 8, 2))
    with pytest.raises(ValueError, match="needs occupancy"):
        render_orbit(rend, torch.nn.Identity(), torch.eye(3), 1, 1.0, 4, ray_bounds="grid")
    with pytest.raises(ValueError, match="must be None or 'grid'"):
        render_orbit(rend, torch.nn.Identity(), torch.eye(3), 1, 1.0, 4, occupancy=32, ray_bounds="cells")


def test_cli_refuses_ray_bounds_without_occupancy(capsys):
    from avr import render
    with pytest.raises(SystemExit):
        render.main(["--ray-bounds", "grid"])
    assert "--ray-bounds needs --occupancy" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        render.main(["--occupancy", "32", "--ray-bounds", "cells"])


def test_ops_refuse_host_tensors_and_mixed_bounds():
    from avr import ops
    from avr._lib import AVRError
    w, z = torch.rand(4, 8), torch.rand(4, 8)
    with pytest.raises(AVRError, match="two floats or two"):
        ops.sample_fine(w, z, torch.zeros(4), 1.8, 4, 0, 0.0)
    with pytest.raises(AVRError, match="entries for 4 rays"):
        ops.sample_fine(w, z, torch.zeros(3), torch.ones(3), 4, 0, 0.0)
    with pytest.raises(AVRError, match="no CPU path"):
        ops.sample_coarse_bounds(torch.zeros(4), torch.ones(4), 8)
    with pytest.raises(AVRError, match="no CPU path"):
        _grid().ray_bounds(torch.zeros(4, 3), torch.ones(4, 3), 0.8, 1.8)


def test_argument_checks_through_ctypes():
    """The refusals of include/avr.h through the product library, with null or host-only arguments: code 1001, the
    entry named in the message; no rays launches nothing and succeeds."""
    from avr import _lib
    lib = _lib.load()
    host = (ctypes.c_double * 8)()
    hp = ctypes.addressof(host)
    err = lambda: lib.avr_last_error_string()  # noqa: E731
    F3, I3 = ctypes.c_float * 3, ctypes.c_int * 3
    g = ctypes.byref(_lib.OccGrid(F3(-1, -1, -1), F3(16, 16, 16), I3(32, 32, 32), hp))
    assert lib.avr_occ_ray_bounds(None, hp, hp, 5, 0.8, 1.8, hp, hp, None) == 1001 and b"null grid" in err()
    assert lib.avr_occ_ray_bounds(g, hp, hp, -1, 0.8, 1.8, hp, hp, None) == 1001 and b"n_rays" in err()
    assert lib.avr_occ_ray_bounds(g, hp, hp, 5, 1.8, 0.8, hp, hp, None) == 1001 and b"near" in err()
    assert lib.avr_occ_ray_bounds(g, hp, hp, 5, float("nan"), 0.8, hp, hp, None) == 1001 and b"near" in err()
    assert lib.avr_occ_ray_bounds(g, None, hp, 5, 0.8, 1.8, hp, hp, None) == 1001 and b"null" in err()
    assert lib.avr_occ_ray_bounds(g, None, None, 0, 0.8, 1.8, None, None, None) == 0
    assert lib.avr_sample_coarse_bounds(None, hp, 5, 32, hp, 0, 0, None, hp, None) == 1001 and b"null" in err()
    assert lib.avr_sample_coarse_bounds(hp, hp, 5, 0, hp, 0, 0, None, hp, None) == 1001 and b"sizes" in err()
    assert lib.avr_sample_coarse_bounds(None, None, 0, 32, None, 0, 0, None, None, None) == 0
    fine = lib.avr_sample_fine_bounds
    assert fine(hp, hp, None, hp, 5, 32, 16, 0, 0.01, hp, hp, None, 0, 0, None, hp, hp, hp, None) == 1001
    assert b"avr_sample_fine_bounds: null bounds" in err()
    assert fine(hp, hp, hp, hp, 5, 257, 16, 0, 0.01, hp, hp, None, 0, 0, None, hp, hp, hp, None) == 1001
    assert b"avr_sample_fine_bounds: n_coarse" in err()
    assert fine(None, None, None, None, 0, 32, 16, 0, 0.01, None, None, None, 0, 0, None, None, None, None, None) == 0
    assert all(v == 0.0 for v in host)


def test_ray_bounds_abi_check_under_host_asan():
    """tests/ray_bounds_abi_check.c against the host-AddressSanitizer build of the library (`make asan-ray-bounds`),
    run as a program of its own: nothing is preloaded and nothing is loaded into Python."""
    b = subprocess.run(["make", "-C", PKG, "asan-ray-bounds", "-j8"], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([os.path.join(PKG, "build", "ray_bounds_abi_check_asan")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "ray_bounds_abi_check: 0 failure(s)" in r.stdout
    assert "AddressSanitizer" not in r.stderr
