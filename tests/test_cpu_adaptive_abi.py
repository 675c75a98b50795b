"""avr_adaptive_front in the C ABI (include/avr.h): exported within ABI 18, bound by avr._lib, and its argument
checks under the host-AddressSanitizer build of the library. No GPU: every check precedes the launch."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "adaptive-volume-rendering_amd")


def test_library_exports_adaptive_front_within_the_abi():
    from avr import _lib
    lib = _lib.load()
    assert "avr_adaptive_front" in _lib.EXPORTED and hasattr(lib, "avr_adaptive_front")
    assert lib.avr_version() == _lib.ABI_VERSION        # an addition: the version did not move
    assert len(_lib._SIGS["avr_adaptive_front"]) == 24   # include/avr.h's parameter list
    header = open(os.path.join(REPO, "include", "avr.h")).read()
    assert "int avr_adaptive_front(" in header and "0x8008" in header and "0x10010" in header


def test_adaptive_abi_check_under_host_asan():
    """tests/adaptive_abi_check.c against the host-AddressSanitizer build of the library (`make asan-adaptive`),
    run as a program of its own: nothing is preloaded and nothing is loaded into Python."""
    b = subprocess.run(["make", "-C", PKG, "asan-adaptive", "-j8"], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([os.path.join(PKG, "build", "adaptive_abi_check_asan")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "adaptive_abi_check: 0 failure(s)" in r.stdout
    assert "AddressSanitizer" not in r.stderr
