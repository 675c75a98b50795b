"""CPU-only checks of occupancy gating with a device-side live count (avr.occupancy, include/avr.h "occupancy grid,
device-side count"; additions within ABI 18): the four entries are exported and bound and refuse bad arguments before
any HIP call, the Python layer refuses what it must without touching a device, and the argument checks pass a host
AddressSanitizer build driven by a stand-alone program. No kernel is launched."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "adaptive-volume-rendering_amd")
ENTRIES = ("avr_occ_scan", "avr_occ_compact_counted", "avr_occ_expand_counted", "avr_field_fwd_points_counted")
INVALID, UNSUPPORTED = 1001, 1002


def test_entries_are_exported_and_bound():
    from avr import _lib
    lib = _lib.load()
    assert lib.avr_version() == 18 == _lib.ABI_VERSION
    header = open(os.path.join(REPO, "include", "avr.h")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTED and hasattr(lib, name) and re.search(rf"\bint {name}\(", header), name
        assert getattr(lib, name).argtypes == _lib._SIGS[name] and getattr(lib, name).restype is ctypes.c_int
    assert int(re.search(r"#define AVR_OCC_SCAN_RAYS (\d+)", header).group(1)) == _lib.OCC_SCAN_RAYS
    # the entries of the host-read chain stay
    for name in ("avr_occ_classify", "avr_occ_compact", "avr_occ_expand", "avr_field_fwd_points"):
        assert name in _lib.EXPORTED and hasattr(lib, name)


def test_argument_checks_without_a_device():
    """Every refusal of include/avr.h through ctypes with null or host-only arguments: the code and the stated
    message; n_rays == 0 and capacity == 0 launch nothing and succeed."""
    from avr import _lib
    lib = _lib.load()
    host = (ctypes.c_double * 8)()          # 8-B aligned at least; + 16 below for the 16-B checks
    base = ctypes.addressof(host)
    hp = (base + 15) & ~15
    odd8, odd16 = hp + 4, hp + 4
    err = lambda: lib.avr_last_error_string()  # noqa: E731
    scan, compact, expand, field = (getattr(lib, n) for n in ENTRIES)

    assert scan(hp, -1, hp, hp, None) == INVALID and b"n_rays" in err()
    assert scan(hp, 4, hp, None, None) == INVALID and b"null" in err()
    assert scan(None, 0, None, None, None) == INVALID and b"null" in err()      # total is always written
    assert scan(None, 4, hp, hp, None) == INVALID and b"null" in err()
    assert scan(hp, 4, None, hp, None) == INVALID and b"null" in err()
    assert scan(hp, 4, hp, odd8, None) == INVALID and b"aligned" in err()
    assert scan(hp, 4, odd8, hp, None) == INVALID and b"aligned" in err()
    assert scan(hp, _lib.OCC_SCAN_RAYS << 31, hp, hp, None) == INVALID and b"too many" in err()

    ok = [hp, hp, hp, hp, hp, 4, 8, hp, 32, hp, hp, None]     # ro rd z mask offsets R N n_live capacity xyz vd stream
    for i in (0, 1, 2, 3, 4, 7, 9, 10):
        a = list(ok)
        a[i] = None
        assert compact(*a) == INVALID and b"null" in err(), i
    for i, v, what in ((7, odd8, b"aligned"), (6, 0, b"n_samples"), (6, 257, b"n_samples"), (5, -4, b"n_rays"),
                       (8, -1, b"capacity"), (8, 33, b"capacity")):
        a = list(ok)
        a[i] = v
        assert compact(*a) == INVALID and what in err(), (i, v)
    assert compact(None, None, None, None, None, 4, 8, None, 0, None, None, None) == 0
    assert compact(None, None, None, None, None, 0, 8, None, 0, None, None, None) == 0

    ok = [hp, hp, hp, 4, 8, hp, 32, hp, None]                # field_c mask offsets R N n_live capacity field stream
    for i in (0, 1, 2, 5, 7):
        a = list(ok)
        a[i] = None
        assert expand(*a) == INVALID and b"null" in err(), i
    for i, v, what in ((5, odd8, b"aligned"), (7, odd16, b"aligned"), (0, odd16, b"aligned"), (4, 0, b"n_samples"),
                       (4, 257, b"n_samples"), (3, -1, b"n_rays"), (6, -1, b"capacity"), (6, 33, b"capacity")):
        a = list(ok)
        a[i] = v
        assert expand(*a) == INVALID and what in err(), (i, v)
    assert expand(None, None, None, 4, 8, None, 0, None, None) == 0
    assert expand(None, None, None, 0, 8, None, 0, None, None) == 0

    d = _lib.FieldDims()
    d.d_in, d.d_latent, d.d_hidden, d.n_blocks, d.n_lin_z, d.num_freqs = 42, 512, 512, 3, 3, 6
    d.freq_factor, d.precision = 1.5, _lib.FIELD_X3
    v = _lib.ViewDesc()
    dp, vp = ctypes.byref(d), ctypes.byref(v)
    assert field(dp, vp, hp, hp, hp, hp, 4, hp, hp, None) == INVALID and b"latent" in err()
    v.latent_h = v.latent_w = 8
    assert field(None, vp, hp, hp, hp, hp, 4, hp, hp, None) == INVALID and b"null" in err()
    ok = [dp, vp, hp, hp, hp, hp, 4, hp, hp, None]          # dims view packed table xyz viewdirs capacity n out stream
    for i in (1, 2, 3, 4, 5, 7, 8):
        a = list(ok)
        a[i] = None
        assert field(*a) == INVALID and b"null" in err(), i
    for i, val, what in ((6, -1, b"capacity"), (8, odd16, b"aligned"), (7, odd8, b"aligned")):
        a = list(ok)
        a[i] = val
        assert field(*a) == INVALID and what in err(), (i, val)
    assert field(dp, vp, hp, hp, None, None, 0, None, None, None) == 0
    for name, val in (("bn", 1), ("spade", 1), ("beta", 1.0)):      # no counted kernel: an error, never another path
        setattr(d, name, val)
        assert field(*ok) == UNSUPPORTED and b"counted" in err(), name
        setattr(d, name, 0)
    assert not any(host)                                             # no refused or empty call wrote anything


def _grid(res=(32, 32, 32), lo=(-1, -1, -1), hi=(1, 1, 1)):
    from avr.occupancy import OccupancyGrid
    return OccupancyGrid.all_occupied(lo, hi, res, "cpu")


def test_occupancy_count_values():
    from avr.renderers import VolumeRenderer
    rend = VolumeRenderer(0.8, 1.8, 128, 64, 0, 0.01, True)
    assert rend.occupancy_count == "host" and rend.last_live_counts is None
    rend.occupancy_count = "device"
    assert rend.occupancy_count == "device"
    for bad in ("bogus", None, "Device", 1):
        with pytest.raises(ValueError, match="occupancy_count"):
            rend.occupancy_count = bad
    assert rend.occupancy_count == "device"
    from avr.occupancy import gated_field
    z = torch.zeros(2, 4)
    with pytest.raises(ValueError, match="count"):
        gated_field(None, _grid(), torch.zeros(2, 3), torch.zeros(2, 3), z, True, count="bogus")


def test_device_mode_keeps_the_refusals_that_need_no_device():
    """autograd, t_stop, the grid count, 256 samples and the fused single-view path are refused in device mode as in
    host mode, before any launch and before the seeded renderer's offset moves."""
    from avr.renderers import VolumeRenderer

    def call(rend, SB=1):
        R = 8
        return rend(torch.eye(4).reshape(1, 1, 4, 4).expand(SB, R, 4, 4), torch.eye(3)[None].expand(SB, 3, 3),
                    torch.rand(SB, R, 2), torch.nn.Identity())

    rend = VolumeRenderer(0.8, 1.8, 128, 64, 0, 0.01, True)
    rend.seed, rend.occupancy, rend.occupancy_count = 5, _grid(), "device"
    with pytest.raises(ValueError, match="no_grad"):
        call(rend)
    with torch.no_grad():
        rend.t_stop = 1e-3
        with pytest.raises(ValueError, match="t_stop"):
            call(rend)
        rend.t_stop = None
        with pytest.raises(ValueError, match=r"1 grid\(s\) for 2 scene"):
            call(rend, SB=2)
        with pytest.raises(ValueError, match="fused path"):
            call(rend)
        big = VolumeRenderer(0.8, 1.8, 200, 100, 0, 0.01, True)
        big.occupancy, big.occupancy_count = _grid(), "device"
        with pytest.raises(ValueError, match="256 samples"):
            call(big)
    assert rend._offset == 0


def test_graphed_renderer_still_refuses_the_host_count():
    from avr.graphs import GraphedRenderer
    from avr.renderers import VolumeRenderer
    rend = VolumeRenderer(0.8, 1.8, 128, 64, 0, 0.01, True)
    rend.occupancy = _grid()
    assert rend.occupancy_count == "host"
    with pytest.raises(ValueError, match="occupancy"):
        GraphedRenderer(rend, torch.nn.Identity(), torch.eye(4).reshape(1, 1, 4, 4), torch.eye(3)[None],
                        torch.rand(1, 8, 2))


def test_cli_occupancy_count_needs_occupancy(capsys):
    from avr import render
    for argv in (["--occupancy-count", "device"], ["--occupancy-count", "host"]):
        with pytest.raises(SystemExit) as e:
            render.main(argv)
        assert e.value.code == 2 and "--occupancy-count needs --occupancy" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        render.main(["--occupancy", "32", "--occupancy-count", "bogus"])
    assert e.value.code == 2 and "--occupancy-count" in capsys.readouterr().err
    from avr.video import render_orbit
    with pytest.raises(ValueError, match="occupancy_count"):
        render_orbit(None, None, torch.eye(3), 1, 1.0, 8, occupancy=32, occupancy_count="bogus")
    with pytest.raises(ValueError, match="needs occupancy"):
        render_orbit(None, None, torch.eye(3), 1, 1.0, 8, occupancy_count="device")


def test_copy_refuses_another_box_or_resolution():
    a = _grid()
    for other in (_grid(res=(64, 32, 32)), _grid(res=(32, 32, 16)), _grid(lo=(-1, -1, -2)), _grid(hi=(1, 2, 1))):
        with pytest.raises(ValueError, match="copy_"):
            a.copy_(other)
    b = _grid()
    b.bits.zero_()
    b.key, b._keep = ("k",), ["kept"]
    addr = a.bits.data_ptr()
    assert a.copy_(b) is a
    assert a.bits.data_ptr() == addr == a.desc.bits and not a.bits.any() and a.live_fraction() == 0.0
    assert a.key == ("k",) and a._keep == ["kept"]
    assert b.bits.data_ptr() != addr


def test_occupancy_count_abi_check_under_host_asan():
    """tests/occupancy_count_abi_check.c against the host-AddressSanitizer build of the library
    (`make asan-occupancy-count`), run as a program of its own: nothing is preloaded and nothing is loaded into
    Python."""
    b = subprocess.run(["make", "-C", PKG, "asan-occupancy-count", "-j8"], capture_output=True, text=True,
                       timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([os.path.join(PKG, "build", "occupancy_count_abi_check_asan")], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "occupancy_count_abi_check: 0 failure(s)" in r.stdout
    assert "AddressSanitizer" not in r.stderr
