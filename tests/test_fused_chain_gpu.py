"""GPU: a frame the fused detection chain cannot hold is redone on the slow path at once.

A regular grid of dots gives thousands of candidates with a handful of distinct response values, so a value bucket gets far
more keys than its 512 slots (kernels.hpp kBucketSlots).  The keys past the slots own no suppression lane; the suppression
must then decide nothing -- no lane may wait for such a candidate until the spin tripwire -- and the frame must come back
from the slow path with the oracle's keypoints, in milliseconds."""
import time

import numpy as np
import pytest

import oracle
from polychase_amd import hip

pytestmark = pytest.mark.gpu


def _dots(w, h, step):
    g = np.zeros((h, w), np.uint8)
    g[4:h - 4:step, 4:w - 4:step] = 200
    return np.repeat(g[:, :, None], 3, axis=2)


def test_overflowing_value_bucket_is_redone_without_waiting():
    w, h = 320, 240
    rgb = _dots(w, h, 4)
    g = oracle.rgb2gray(rgb)
    xy, _, ncand = oracle.gftt(g, want_eig=True)
    e = oracle.min_eigen_val(g)
    assert ncand > 4 * 512 and np.unique(e[e > 0.01 * e.max()]).size < 16, "the frame must overflow a value bucket"
    ctx = hip.Context(0)
    f = hip.Frame(ctx, w, h)
    f.set_rgb(rgb)
    f.detect()                       # first call: the slow path's buffers are allocated here
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        f.detect()
        times.append(time.perf_counter() - t0)
        assert f.num_candidates == ncand
        assert np.array_equal(f.keypoints(), xy), "keypoints must match in value AND order"
    # a suppression that waited for an unowned candidate would sit out the spin tripwire (> 0.1 s per call)
    assert min(times) < 0.1, f"detection of an overflowing frame took {min(times) * 1e3:.1f} ms"
    f.close()
    ctx.close()
