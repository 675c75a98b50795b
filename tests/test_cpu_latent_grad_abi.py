"""avr_latent_features_adjoint and its scratch-size query in the C ABI (include/avr.h): exported within ABI 18,
bound by avr._lib, and their argument checks under the host-AddressSanitizer build of the library. No GPU: every
check precedes the first launch."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "adaptive-volume-rendering_amd")
ENTRIES = ("avr_latent_features_adjoint_scratch_bytes", "avr_latent_features_adjoint")


def test_library_exports_latent_adjoint_within_the_abi():
    from avr import _lib
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "avr.h")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTED and hasattr(lib, name)
        assert f"int {name}(" in header
    assert lib.avr_version() == _lib.ABI_VERSION == 18      # an addition: the version did not move
    assert len(_lib._SIGS["avr_latent_features_adjoint_scratch_bytes"]) == 6   # include/avr.h's parameter lists
    assert len(_lib._SIGS["avr_latent_features_adjoint"]) == 11
    chunk = re.search(r"#define AVR_LATENT_ADJOINT_CHUNK (\d+)", header)
    assert chunk and int(chunk.group(1)) == _lib.LATENT_ADJOINT_CHUNK


def test_latent_grad_abi_check_under_host_asan():
    """tests/latent_grad_abi_check.c against the host-AddressSanitizer build of the library
    (`make asan-latent-grad`), run as a program of its own: nothing is preloaded and nothing is loaded into Python."""
    b = subprocess.run(["make", "-C", PKG, "asan-latent-grad", "-j8"], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([os.path.join(PKG, "build", "latent_grad_abi_check_asan")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "latent_grad_abi_check: 0 failure(s)" in r.stdout
    assert "AddressSanitizer" not in r.stderr
