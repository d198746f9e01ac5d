"""The present pass's pinned sampling rule in numpy (include/hip_raytrace.h hrt_present):
shared by tests/test_present_abi.py (properties of the mapping, CPU) and tests/test_gpu_present.py (the
expected bytes of every target)."""
import numpy as np

B8G8R8A8, R8G8B8A8 = 0, 1  # hrt_present_format


def source_index(ws: int, hs: int, wt: int, ht: int):
    """(sx[wt], sy[ht]): the source texel of each target column / row.  Sample points at the target's
    pixel centres, nearest filter, flipped vertically:
    sx = ((2x+1) ws) div (2 wt),  sy = hs - 1 - ((2y+1) hs) div (2 ht)  (Python ints: no overflow)."""
    sx = np.array([((2 * x + 1) * ws) // (2 * wt) for x in range(wt)], dtype=np.int64)
    sy = np.array([hs - 1 - ((2 * y + 1) * hs) // (2 * ht) for y in range(ht)], dtype=np.int64)
    return sx, sy


def present_pixels(src: np.ndarray, wt: int, ht: int, fmt: int) -> np.ndarray:
    """src: (hs, ws, 4) uint8 RGBA -> the target's (ht, wt, 4) bytes."""
    hs, ws = src.shape[:2]
    sx, sy = source_index(ws, hs, wt, ht)
    out = src[sy[:, None], sx[None, :]]
    if fmt == B8G8R8A8:
        out = out[..., [2, 1, 0, 3]]
    return np.ascontiguousarray(out)


def present_bytes(src: np.ndarray, wt: int, ht: int, pitch: int, fmt: int, total: int, offset: int = 0,
                  fill: int = 0xA5) -> np.ndarray:
    """The whole target allocation of `total` bytes pre-filled with `fill`, after a present of src into
    the wt x ht target that starts at byte `offset` with rows `pitch` bytes apart: pad bytes and
    everything around the rows keep the fill."""
    raw = np.full(total, fill, np.uint8)
    px = present_pixels(src, wt, ht, fmt).reshape(ht, wt * 4)
    for y in range(ht):
        raw[offset + y * pitch: offset + y * pitch + wt * 4] = px[y]
    return raw
