"""The fold record and the settle rule in numpy (include/hip_raytrace.h): the reference the
fold-record tests build every expected value from.  Nothing here touches the library under test
(oracle_records runs the CPU oracle alone)."""
from __future__ import annotations

import functools

import numpy as np

ANY = 0xFFFFFFFF  # a disabled bound of the rule


def records(before: np.ndarray, after: np.ndarray):
    """(changed_pixels, abs_delta_sum, max_delta) of one fold: before / after are the DISPLAYED images
    (uint8, (..., 4)) over the real pixels only."""
    assert before.dtype == np.uint8 and after.dtype == np.uint8 and before.shape == after.shape
    assert before.shape[-1] == 4
    d = np.abs(after.astype(np.int64) - before.astype(np.int64)).reshape(-1, 4)
    if d.size == 0:
        return 0, 0, 0
    return int((d != 0).any(axis=1).sum()), int(d.sum()), int(d.max())


def quiet(rec, max_changed_pixels=ANY, max_delta=ANY) -> bool:
    """rec = (changed_pixels, abs_delta_sum, max_delta): both bounds must hold."""
    return rec[0] <= max_changed_pixels and rec[2] <= max_delta


def stop_frame(recs, max_frames, max_changed_pixels=ANY, max_delta=ANY, quiet_frames=1):
    """(frames_done, settled) of hrt_compute_until over the records r_1, r_2, ... of a call: the smallest
    m >= quiet_frames with r_(m - quiet_frames + 1) .. r_m all quiet when m <= max_frames, else
    (max_frames, False).  recs must hold at least min(max_frames, m) records."""
    assert quiet_frames >= 1
    run = 0
    for m in range(1, max_frames + 1):
        run = run + 1 if quiet(recs[m - 1], max_changed_pixels, max_delta) else 0
        if run >= quiet_frames:
            return m, True
    return max_frames, False


@functools.lru_cache(maxsize=None)
def oracle_records(scene="island", size=(96, 64), spp=3, bounces=8, frames=24):
    """The oracle alone: frames 1..frames of the scene folded into a cleared rgba8 accumulator by the
    oracle's combiner; one (changed_pixels, abs_delta_sum, max_delta) per frame."""
    import pyoracle
    from helpers import SceneCase
    case = SceneCase(scene, size, spp, bounces)
    acc = np.zeros((size[1], size[0], 4), np.uint8)
    pyoracle.accumulate_rgba8(0, acc, acc.copy())
    recs = []
    for k in range(1, frames + 1):
        before = acc.copy()
        pyoracle.accumulate_rgba8(k, acc, case.oracle(rng_offset=k)[0])
        recs.append(records(before, acc))
    return tuple(recs)
