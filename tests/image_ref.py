"""The image passes in numpy float32 (include/hip_raytrace.h hrt_accumulate): the
UNORM8 store and load, the progressive combiner in both accumulator formats, the displayed image and the
fold record -- a few lines each, written from the specification and independent of the C oracle
(tests/test_image_ref.py pins them to it on the CPU).  tests/test_gpu_image_exhaustive.py builds every
expected byte from these.  numpy's float32 arithmetic rounds every operation on its own (no contraction), and
its division is IEEE's: x / 0 is an infinity or a NaN, with the warnings silenced."""
from __future__ import annotations

import numpy as np

F32 = np.float32


def unorm8(x) -> np.ndarray:
    """S7, the R8G8B8A8_UNORM store: NaN or x <= 0 gives 0, x >= 1 gives 255, else rint(x * 255) in
    float32 (round to nearest, ties to even)."""
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        r = np.rint(x * F32(255))
        inside = (x > 0) & (x < 1)
        r = np.where(inside, r, F32(0))
        return np.where(x >= 1, 255, r.astype(np.int64)).astype(np.uint8)


def unorm8_to_float(k) -> np.ndarray:
    """The UNORM8 load: float32(k) / float32(255)."""
    return np.asarray(k).astype(F32) / F32(255)


def _denominators(frame: int):
    frame = int(frame) & 0xFFFFFFFF
    return frame, F32(frame), F32((frame + 1) & 0xFFFFFFFF)


def fold_rgba8(frame: int, cur: np.ndarray, new: np.ndarray) -> np.ndarray:
    """image_combiner.glsl on UNORM8 texels (uint8, (..., 4)): the accumulator after folding `new` in as
    frame `frame`.  Frame 0 clears; the frame whose frame + 1 wraps to 0 divides by zero as IEEE does."""
    assert cur.dtype == np.uint8 and new.dtype == np.uint8 and cur.shape == new.shape and cur.shape[-1] == 4
    frame, ff, ff1 = _denominators(frame)
    out = np.empty_like(cur)
    out[..., 3] = 255
    if frame == 0:
        out[..., :3] = 0
        return out
    with np.errstate(all="ignore"):
        out[..., :3] = unorm8((unorm8_to_float(new[..., :3]) + unorm8_to_float(cur[..., :3]) * ff) / ff1)
    return out


def fold_rgba32f(frame: int, cur: np.ndarray, new: np.ndarray) -> np.ndarray:
    """The same fold on float32 texels, without quantization; alpha 1.0."""
    assert cur.dtype == F32 and new.dtype == F32 and cur.shape == new.shape and cur.shape[-1] == 4
    frame, ff, ff1 = _denominators(frame)
    out = np.empty_like(cur)
    out[..., 3] = 1.0
    if frame == 0:
        out[..., :3] = 0.0
        return out
    with np.errstate(all="ignore"):
        out[..., :3] = (new[..., :3] + cur[..., :3] * ff) / ff1
    return out


def displayed(img: np.ndarray) -> np.ndarray:
    """What hrt_read_image(HRT_FMT_RGBA8), the present pass and the fold records show of an image: the
    bytes themselves, or unorm8 of every channel of a float32 image."""
    if img.dtype == np.uint8:
        return img
    assert img.dtype == F32
    return unorm8(img)


def record(before: np.ndarray, after: np.ndarray, real_rows=None):
    """S10: (changed_pixels, abs_delta_sum, max_delta) of one fold over the displayed words of the first
    real_rows rows (None: every row) of before / after, (rows, W, 4) images of either format."""
    b, a = displayed(before), displayed(after)
    assert b.shape == a.shape and b.shape[-1] == 4
    if real_rows is not None:
        b, a = b[:real_rows], a[:real_rows]
    d = np.abs(a.astype(np.int64) - b.astype(np.int64)).reshape(-1, 4)
    if d.size == 0:
        return 0, 0, 0
    return int((d != 0).any(axis=1).sum()), int(d.sum()), int(d.max())


def same_floats(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Elementwise: the same 32-bit pattern, or both NaN (whatever their sign and payload)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _bits(patterns) -> np.ndarray:
    return np.asarray(patterns, np.uint32).view(F32)


def float_pool() -> np.ndarray:
    """The adversarial float32 values, from bit patterns (the same on every run), specials first:
      +-0, the smallest and largest denormals of both signs, +-FLT_MIN, +-FLT_MAX, +-inf, quiet NaNs of
      both signs, a quiet NaN with a payload, a signalling NaN, 0.5, 2, -1, 1e-10                      (20)
      for k = 0..254: f32((k + 0.5) / 255), where unorm8 rounds between k and k + 1, and its neighbours at
      +-1 and +-2 ulp                                                                               (1,275)
      for k = 1..255: f32(k / 255) and +-1 ulp                                                        (765)
    2,060 values.  (Positive floats are ordered like their bit patterns, so +-n ulp is +-n on the pattern.)"""
    special = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000,
               0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7FC00001, 0x7F800001]
    misc = np.array([0.5, 2.0, -1.0, 1e-10], F32).view(np.uint32)
    k = np.arange(255, dtype=np.float64)
    ties = ((k + 0.5) / 255).astype(F32).view(np.uint32).astype(np.int64)
    ties = (ties[:, None] + np.array([0, -1, 1, -2, 2])[None, :]).reshape(-1)
    k = np.arange(1, 256, dtype=np.float64)
    steps = (k / 255).astype(F32).view(np.uint32).astype(np.int64)
    steps = (steps[:, None] + np.array([0, -1, 1])[None, :]).reshape(-1)
    return _bits(np.concatenate([np.array(special, np.int64), misc.astype(np.int64), ties, steps]).astype(np.uint32))


# ---- the all-pairs inputs (shared by tests/test_image_ref.py and tests/test_gpu_image_exhaustive.py) ----

def column_bytes(n: int = 256) -> np.ndarray:
    """(n, 3): the trace image's colour bytes of column x: (x, (37 x + 11) mod 256, 255 - x)."""
    x = np.arange(n, dtype=np.int64)
    return np.stack([x, (37 * x + 11) % 256, 255 - x], -1).astype(np.uint8)


def row_bytes(n: int = 256) -> np.ndarray:
    """(n, 4): the loaded accumulator's bytes of row y: (y, (91 y + 5) mod 256, 255 - y, (3 y) mod 256)."""
    y = np.arange(n, dtype=np.int64)
    return np.stack([y, (91 * y + 5) % 256, 255 - y, (3 * y) % 256], -1).astype(np.uint8)


def pairs_images(w: int = 256, h: int = 256):
    """(accumulator, trace image), (h, w, 4) uint8: at 256 x 256 every (accumulator byte, trace byte) pair
    occurs in every colour channel (37, 91 and -1 are odd: each channel is a permutation of the bytes)."""
    acc = np.broadcast_to(row_bytes(h)[:, None, :], (h, w, 4)).copy()
    trace = np.full((h, w, 4), 255, np.uint8)
    trace[..., :3] = column_bytes(w)[None, :, :]
    return acc, trace


def assert_all_pairs(acc: np.ndarray, trace: np.ndarray) -> None:
    """The premise of an exhaustive RGBA8 case, on the bytes it is about to use: in each colour channel the
    set of (accumulator byte, trace byte) pairs over the image has 65,536 members."""
    for ch in range(3):
        pairs = acc[..., ch].astype(np.uint32).reshape(-1) * 256 + trace[..., ch].reshape(-1)
        assert len(np.unique(pairs)) == 65536, ch


def fold_rgba8_by_pairs(frame: int, cur: np.ndarray, new: np.ndarray) -> np.ndarray:
    """fold_rgba8 for callers that fold many frames: fold_rgba8 itself over the 65,536 channel pairs (packed
    three to a pixel), gathered per channel -- a third of the arithmetic on a 256 x 256 image, the same bytes
    (tests/test_image_ref.py pins it to the oracle on every frame of F_ALL)."""
    p = np.zeros(65538, np.int64)
    p[:65536] = np.arange(65536)
    c4, n4 = np.zeros((21846, 4), np.uint8), np.zeros((21846, 4), np.uint8)
    c4[:, :3], n4[:, :3] = (p >> 8).reshape(-1, 3), (p & 255).reshape(-1, 3)
    tab = fold_rgba8(frame, c4, n4)[:, :3].reshape(-1)[:65536].reshape(256, 256)
    out = np.empty_like(cur)
    out[..., 3] = 255
    out[..., :3] = tab[cur[..., :3], new[..., :3]]
    return out


LARGE_FRAMES = (2**24 - 1, 2**24, 2**24 + 1, 2**31 - 1, 2**31, 2**32 - 3, 2**32 - 2, 2**32 - 1)
F_ALL = tuple(range(1200)) + LARGE_FRAMES
F_SOME = (0, 1, 2, 3, 15, 16, 254, 255, 256, 509, 510, 511, 1199) + LARGE_FRAMES
