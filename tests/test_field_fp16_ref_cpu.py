"""CPU checks for the field's "fp16" precision. tests/field_fp16_ref.py, the reference the precision is judged against
(tests/test_gpu_field_fp16.py): its exact mode is the reference's field, its rounded mode is visibly rounded and
rightly scaled, and the scale's grouping does not matter. The Python names and the eligibility rules that need no
device. AVR_FIELD_FP16's argument checks under a host AddressSanitizer build, driven by a stand-alone program. No
kernel is launched."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_fp16_ref as ref  # noqa: E402
from conftest import load_golden  # noqa: E402
from helpers import oracle_field  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "adaptive-volume-rendering_amd")
TAGS = ("small", "small_mv", "full", "mv512", "d256")


@pytest.fixture(scope="module")
def cases():
    """tag -> (golden, {mode: {coarse: out}}): each field evaluated once for every test of this module."""
    out = {}
    for tag in TAGS:
        g = load_golden(f"g4_field_{tag}.npz")
        f = oracle_field(g)
        res = {mode: {c: ref.RefField(f, mode)(g["xyz"], g["viewdirs"], coarse=c) for c in (True, False)}
               for mode in ("f64", "e16")}
        out[tag] = (g, f, res)
    return out


def _gold(g, coarse):
    return g["out_coarse" if coarse else "out_fine"]


@pytest.mark.parametrize("tag", TAGS)
def test_f64_mode_reproduces_the_goldens(cases, tag):
    g, _, res = cases[tag]
    for coarse in (True, False):
        err = np.abs(res["f64"][coarse] - _gold(g, coarse)).max()
        print(f"{tag} coarse={coarse}: f64 max err {err:.3e}")
        assert err <= 1e-5, (tag, coarse, err)


@pytest.mark.parametrize("tag", TAGS)
def test_e16_mode_is_rounded_and_rightly_scaled(cases, tag):
    g, _, res = cases[tag]
    for coarse in (True, False):
        e64 = ref.errors(res["f64"][coarse], _gold(g, coarse))
        e16 = ref.errors(res["e16"][coarse], _gold(g, coarse))
        print(f"{tag} coarse={coarse}: f64 (rgb mean, rgb max, sigma mean, sigma max) {e64}  e16 {e16}")
        assert e16[0] >= 10 * e64[0] and e16[1] >= 10 * e64[1], (tag, coarse, e64, e16)   # the rounding is live
        assert e16[1] < 1e-2, (tag, coarse, e16)                                             # the scale is right


@pytest.mark.parametrize("tag", ("small", "full"))
def test_scale_grouping_is_immaterial(cases, tag):
    """One scale per 64 rows (the kernels' workgroups) or one per tensor: bit-identical, because a power-of-two scale
    commutes with rounding to nearest outside the subnormal range."""
    g, f, res = cases[tag]
    by64 = ref.RefField(f, "e16", rows_per_scale=64)(g["xyz"], g["viewdirs"], coarse=False)
    assert np.array_equal(by64, res["e16"][False])


def test_round_fp16_is_nearest_even_under_a_power_of_two_scale():
    # max 3.0 -> scale 2^13 / 2 ... the tensor's max lands in [2^13, 2^14); 11 significant bits survive
    x = np.array([3.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -10, -(1.0 + 2.0 ** -11), 0.0])
    y = ref.round_fp16(x)
    # ties go to the even significand: 1 + 2^-11 -> 1, 1 + 3 * 2^-11 -> 1 + 2^-9 ... (1 + 2^-10 is representable)
    assert y.tolist() == [3.0, 1.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -10, -1.0, 0.0]
    assert np.array_equal(ref.round_fp16(x * 2.0 ** 40), y * 2.0 ** 40)       # scale invariance
    assert np.array_equal(ref.round_fp16(np.zeros(4)), np.zeros(4))


def test_python_names_and_routes_without_a_device():
    from avr import _lib
    from avr.field import PRECISIONS, FusedField, blob_precision
    assert _lib.FIELD_FP16 == 2 and PRECISIONS == {"fp32": 0, "x3": 1, "fp16": 2}
    assert _lib.load().avr_version() == 18 == _lib.ABI_VERSION
    assert [blob_precision(p) for p in ("x3", "fp16", "fp32")] == ["x3", "x3", "fp32"]
    assert FusedField(None, "fp16").precision == "fp16"
    with pytest.raises(ValueError):
        FusedField(None, "bf16")
    header = open(os.path.join(REPO, "include", "avr.h")).read()
    assert "#define AVR_FIELD_FP16 2" in header and "#define AVR_ABI_VERSION 18" in header
    from avr import render
    with pytest.raises(SystemExit):
        render.main(["--precision", "fp8"])


def test_eligibility_under_fp16_without_a_device():
    """ReLU nets fuse under fp16; BatchNorm, use_spade, Softplus and NS > 1 nets do not (module path), while a call
    that needs gradients is routed as under x3."""
    from avr.field import fused_eligible
    from helpers import build_net
    for tag, fusable in (("small", True), ("bn_small", False), ("spade_small", False), ("sp_small", False)):
        net = build_net(load_golden(f"g4_field_{tag}.npz"), "cpu", "fp16")
        assert fused_eligible(net) is fusable, tag
        net.field_precision = "x3"
        assert fused_eligible(net), tag
        x3_train = fused_eligible(net, train=True)
        net.field_precision = "fp16"
        assert fused_eligible(net, train=True) is x3_train, tag
    net = build_net(load_golden("g4_field_ns2_small.npz"), "cpu", "fp16")
    assert not fused_eligible(net) and not fused_eligible(net, multiview=True)
    assert fused_eligible(net, multiview=True, train=True)
    net.field_precision = "x3"
    assert fused_eligible(net, multiview=True)


def test_field_fp16_abi_check_under_host_asan():
    """tests/field_fp16_abi_check.c against the host-AddressSanitizer build of the library (`make asan-field-fp16`),
    run as a program of its own: nothing is preloaded and nothing is loaded into Python."""
    b = subprocess.run(["make", "-C", PKG, "asan-field-fp16", "-j8"], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([os.path.join(PKG, "build", "field_fp16_abi_check_asan")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "field_fp16_abi_check: 0 failure(s)" in r.stdout
    assert "AddressSanitizer" not in r.stderr
