"""The tile-masked refinement in numpy (hrt_refine_tiles, hrt_refine_tiles_until), written from the
specification and independent of the kernels: which 8x8 tiles a selection touches, the pixels a pass traces, the counts
hrt_refine_tiles_stats reports, and the chain of passes of several frames each.  The folds are tests/refine_ref.py's."""
import numpy as np

import refine_ref as R


def tile_mask(sel: np.ndarray) -> np.ndarray:
    """(tiles_y, tiles_x) bool: the 8x8 tiles of an (h, w) bool selection that hold at least one selected pixel (the
    tiles of the right and bottom edges hold fewer than 64 real pixels)."""
    h, w = sel.shape
    ty, tx = (h + 7) // 8, (w + 7) // 8
    pad = np.zeros((ty * 8, tx * 8), bool)
    pad[:h, :w] = sel
    return pad.reshape(ty, 8, tx, 8).any(axis=(1, 3))


def traced_pixels(sel: np.ndarray) -> np.ndarray:
    """(h, w) bool: the real pixels of the selected tiles -- every pixel a tile-masked pass traces."""
    h, w = sel.shape
    return np.repeat(np.repeat(tile_mask(sel), 8, axis=0), 8, axis=1)[:h, :w]


def tile_bit_words(sel: np.ndarray) -> np.ndarray:
    """The tile bitmap's words: tile t = tx + ty tiles_x is bit t & 31 of word t >> 5."""
    return R.pack_mask(tile_mask(sel))


def counts(sel: np.ndarray):
    """(tiles, tiles_selected, selected, pixels_traced) of hrt_refine_tiles_stats for a masked pass."""
    t = tile_mask(sel)
    return int(t.size), int(t.sum()), int(sel.sum()), int(traced_pixels(sel).sum())


def refine_tiles(acc, cnt, mom, frames, sel, max_history: int, moments: bool = True):
    """hrt_refine_tiles: `frames` (a sequence of trace images, rng_offset, + 1, ...) folded in order into the selected
    pixels, each as one hrt_refine pass folds it.  (acc', cnt', mom')."""
    for frame in frames:
        acc, cnt, mom = R.refine(acc, cnt, mom, frame, sel, max_history, moments)
    return acc, cnt, mom


def refine_tiles_until(acc, cnt, mom, frames, max_history: int, max_passes: int, frames_per_pass: int, key=None,
                       rule=R.DEFAULTS):
    """hrt_refine_tiles_until: frames(j) = the trace image of rng_offset + j; pass k selects once, then folds the
    frames k frames_per_pass .. (k + 1) frames_per_pass - 1.  Returns (acc, cnt, mom, passes, pixel_frames, settled,
    selected per pass)."""
    passes, pixel_frames, settled, selected = 0, 0, False, []
    for k in range(max_passes):
        sel = R.select(cnt, mom, key, *rule)
        n = int(sel.sum())
        if n == 0:
            settled = True
            break
        selected.append(n)
        acc, cnt, mom = refine_tiles(acc, cnt, mom, [frames(k * frames_per_pass + f) for f in range(frames_per_pass)],
                                     sel, max_history, True)
        passes += 1
        pixel_frames += n * frames_per_pass
    return acc, cnt, mom, passes, pixel_frames, settled, selected
