"""CPU restatement of the two Philox streams of avr_adaptive_front (include/avr.h), on oracle.philox.uniform4
(test infrastructure only): the LSTM march's start distance (stream 0x8008) and the adaptive band's noise
(stream 0x10010). `keys` are the per-ray counters oracle.philox.ray_keys builds (offset + frame-wide ray id)."""
import numpy as np

from oracle import philox

STREAM_MARCH, STREAM_BAND = 0x8008, 0x10010


def band_noise(seed, keys, n):
    """The band's sample_coarse draw (renderers.py:14 as called at :492): (R, n) float32, sample i = word i & 3 of
    block i >> 2 (the first n values of the row-major quads)."""
    nq = (n + 3) // 4
    v = philox.uniform4(seed, keys, np.arange(nq), STREAM_BAND)
    return np.ascontiguousarray(v.reshape(len(keys), nq * 4)[:, :n])


def init_distance(seed, keys):
    """The start distance normal_(mean=0.8, std=5e-2) (renderers.py:322 / :402): (R,) float64, 0.8 + 0.05 *
    Box-Muller on words 0, 1 of block 0, in float64 as oracle.philox.depth_normal restates the kernel's
    Box-Muller (its logf / cospif are not restated bit for bit)."""
    v = philox.uniform4(seed, keys, np.arange(1), STREAM_MARCH).astype(np.float64)[:, 0]
    u1 = np.maximum(v[:, 0], 1e-7)
    return 0.8 + 0.05 * (np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * v[:, 1]))
