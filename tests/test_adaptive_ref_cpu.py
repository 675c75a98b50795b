"""tests/adaptive_ref.py: the CPU restatement of avr_adaptive_front's two Philox streams is deterministic, disjoint
from the three streams of the sampling kernels, and keyed by offset + frame-wide ray id."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_ref  # noqa: E402
from oracle import philox  # noqa: E402


def test_draws_are_deterministic_and_in_range():
    keys = philox.ray_keys(50, offset=1000)
    a, b = adaptive_ref.band_noise(99, keys, 7), adaptive_ref.band_noise(99, keys, 7)
    assert a.dtype == np.float32 and a.shape == (50, 7) and np.array_equal(a, b)
    assert float(a.min()) >= 0.0 and float(a.max()) < 1.0
    d, e = adaptive_ref.init_distance(99, keys), adaptive_ref.init_distance(99, keys)
    assert d.dtype == np.float64 and d.shape == (50,) and np.array_equal(d, e)
    assert not np.array_equal(a, adaptive_ref.band_noise(100, keys, 7))            # the seed matters
    assert not np.array_equal(d, adaptive_ref.init_distance(100, keys))
    # the first n values of the row-major quads: a shorter band is a prefix of a longer one
    assert np.array_equal(adaptive_ref.band_noise(99, keys, 20)[:, :7], a)
    # normal_(mean=0.8, std=5e-2): 4096 draws land within 6 sigma, with the right first two moments
    big = adaptive_ref.init_distance(3, philox.ray_keys(4096))
    assert float(np.abs(big - 0.8).max()) < 6 * 0.05
    assert abs(float(big.mean()) - 0.8) < 5 * 0.05 / 64 and abs(float(big.std()) - 0.05) < 0.005


def test_streams_are_disjoint_from_the_sampling_kernels():
    keys = philox.ray_keys(16, offset=5)
    band = adaptive_ref.band_noise(7, keys, 8)
    assert not np.array_equal(band, philox.coarse_noise(7, keys, 8))
    u, u2 = philox.fine_noise(7, keys, 8)
    assert not np.array_equal(band, u) and not np.array_equal(band, u2)
    assert len({adaptive_ref.STREAM_MARCH, adaptive_ref.STREAM_BAND, philox.STREAM_COARSE, philox.STREAM_FINE,
                philox.STREAM_DEPTH}) == 5
    # the start distance is not the depth stream's normal either
    d = (adaptive_ref.init_distance(7, keys) - 0.8) / 0.05
    assert not np.allclose(d, philox.depth_normal(7, keys, 1)[:, 0], atol=1e-6)
    # nor do the two new streams share words: the march's quad 0 is not the band's
    first = philox.uniform4(7, keys, np.arange(1), adaptive_ref.STREAM_MARCH)[:, 0]
    assert not np.array_equal(first, adaptive_ref.band_noise(7, keys, 4))


def test_keys_honour_offset_and_ray_ids():
    ids = np.array([40, 3, 17, 1000, 5], np.uint64)          # a permutation with gaps
    keys = philox.ray_keys(5, offset=1000, ray_ids=ids)
    full = philox.ray_keys(1001, offset=1000)
    a, d = adaptive_ref.band_noise(99, keys, 7), adaptive_ref.init_distance(99, keys)
    assert np.array_equal(a, adaptive_ref.band_noise(99, full, 7)[ids.astype(np.int64)])
    assert np.array_equal(d, adaptive_ref.init_distance(99, full)[ids.astype(np.int64)])
    # offset + id is all that matters: ray 3 at offset 1000 is ray 0 at offset 1003
    assert np.array_equal(a[1], adaptive_ref.band_noise(99, philox.ray_keys(1, offset=1003), 7)[0])
    assert not np.array_equal(a, adaptive_ref.band_noise(99, philox.ray_keys(5, offset=0, ray_ids=ids), 7))
