"""tests/image_ref.py against the CPU oracle: the numpy restatement of the combiner and the UNORM8 store that
tests/test_gpu_image_exhaustive.py holds the device to is the oracle's arithmetic, on every input those
tests use -- all 65,536 channel pairs at every frame of F_ALL, and the whole float pool."""
import numpy as np

import image_ref
import pyoracle


def test_pool_is_what_the_tests_assume():
    pool = image_ref.float_pool()
    bits = pool.view(np.uint32)
    assert pool.dtype == np.float32 and len(pool) == 2060
    assert len(np.unique(bits[:256])) == 256  # the emissions of the float sphere scene are 256 different values
    assert {0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00001,
            0x7F800001} <= set(int(b) for b in bits[:256])
    assert int(np.isnan(pool).sum()) == 4
    with np.errstate(all="ignore"):
        prod = pool * np.float32(255)
        ties = int(((prod - np.floor(prod)) == np.float32(0.5)).sum())
    assert ties == 257  # values whose float32 product with 255 is an exact tie for rint
    assert len(np.unique(image_ref.unorm8(pool))) == 256  # every byte is reached


def test_unorm8_matches_the_oracle_on_the_pool():
    pool = image_ref.float_pool()
    want = np.array([pyoracle.unorm8(float(v)) for v in pool], np.uint8)
    got = image_ref.unorm8(pool)
    assert np.array_equal(got, want), pool[got != want][:8]
    assert np.array_equal(image_ref.unorm8_to_float(np.arange(256)).view(np.uint32),
                          (np.arange(256, dtype=np.float32) / np.float32(255)).view(np.uint32))


def test_fold_rgba8_matches_the_oracle_on_all_pairs():
    """fold_rgba8, and fold_rgba8_by_pairs (what the device's F_ALL sweep is compared with), on every
    (accumulator byte, trace byte) pair in every colour channel, every frame of F_ALL -- the wrap
    frame 2^32 - 1 included, where the oracle divides by zero: only the bytes 0 and 255 come out, and 0 only
    at the (0, 0) pairs."""
    acc, trace = image_ref.pairs_images()
    image_ref.assert_all_pairs(acc, trace)
    for frame in image_ref.F_ALL:
        want = acc.copy()
        pyoracle.accumulate_rgba8(frame, want, trace)
        got = image_ref.fold_rgba8(frame, acc, trace)
        assert np.array_equal(got, want), frame
        assert np.array_equal(image_ref.fold_rgba8_by_pairs(frame, acc, trace), want), frame
    assert set(np.unique(want[..., :3])) == {0, 255}
    assert np.array_equal(want[..., :3] == 0, (acc[..., :3] == 0) & (trace[..., :3] == 0))


def test_fold_rgba32f_matches_the_oracle_on_pool_pairs():
    """pool x pool samples: 2,060 accumulator values (alpha included) against 206 trace values each, over the
    frames of the GPU cases; NaNs compare as "both NaN"."""
    pool = image_ref.float_pool()
    n = len(pool)
    i, j = np.meshgrid(np.arange(n), np.arange(0, n, 10), indexing="ij")
    cur = np.stack([pool[i], pool[(i + 7) % n], pool[(i + 1031) % n], pool[(i + 3) % n]], -1)
    new = np.stack([pool[j], pool[(j + 517) % n], pool[(n - 1 - j)], pool[(j + 5) % n]], -1)
    for frame in (0, 1, 2, 3, 255, 2**24 + 1, 2**32 - 2, 2**32 - 1):
        want = cur.copy()
        pyoracle.accumulate_rgba32f(frame, want, new)
        got = image_ref.fold_rgba32f(frame, cur, new)
        assert image_ref.same_floats(got, want).all(), frame


def test_record_and_displayed():
    a = np.zeros((2, 3, 4), np.uint8)
    b = a.copy()
    b[0, 1] = (5, 0, 250, 0)
    b[1, 2, 3] = 1
    assert image_ref.record(a, b) == (2, 256, 250) and image_ref.record(a, a) == (0, 0, 0)
    assert image_ref.record(a, b, real_rows=1) == (1, 255, 250)
    f = np.array([[[0.5, np.nan, 2.0, -1.0], [0.25, np.inf, -np.inf, 1.0]]], np.float32)
    assert image_ref.displayed(f).tolist() == [[[128, 0, 255, 0], [64, 255, 0, 255]]]
    assert image_ref.record(np.zeros_like(f), f) == (2, 128 + 255 + 64 + 255 + 255, 255)
