"""The mask arithmetic of the tile-masked refinement on the CPU: the HIP-free header the refine_tile_bits kernel shares
(epq_raytracer_amd/csrc/hrt_refine_tile_bits.h) against a bit-by-bit loop in a plain C++ program
(tests/cpp/refine_tile_bits_test.cpp), once more under AddressSanitizer and UBSan as a stand-alone host program, and the
numpy restatement tests/refine_tiles_ref.py against the header on the same kinds of masks."""
import os
import subprocess

import numpy as np

import refine_ref as R
import refine_tiles_ref as T

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")


def build(target):
    subprocess.run(["make", "-s", "-C", CPP, "-f", "refine_tiles_demo.mk", target], check=True)
    return os.path.join(CPP, target)


def test_header_against_the_bit_by_bit_loop():
    r = subprocess.run([build("refine_tile_bits_test")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "masks agree" in r.stdout and int(r.stdout.split()[1]) > 700000, r.stdout


def test_header_under_the_sanitizers():
    r = subprocess.run([build("refine_tile_bits_test_san")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "masks agree" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]


def cases():
    """(w, h, selection): every width 1..70 and height 1..17 all zero, all one and random; a single bit at every
    position for the sizes around the word and tile edges."""
    rng = np.random.default_rng(5)
    for w in range(1, 71):
        for h in range(1, 18):
            yield w, h, np.zeros((h, w), bool)
            yield w, h, np.ones((h, w), bool)
            yield w, h, rng.uniform(size=(h, w)) < 0.5
            yield w, h, rng.uniform(size=(h, w)) < 0.03
    for w, h in ((1, 1), (7, 5), (8, 8), (9, 9), (31, 3), (33, 2), (37, 17), (64, 9), (70, 17)):
        for i in range(w * h):
            sel = np.zeros(w * h, bool)
            sel[i] = True
            yield w, h, sel.reshape(h, w)


def test_numpy_restatement_against_the_header(tmp_path):
    exe = build("refine_tile_bits_test")
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    all_cases = list(cases())
    rng = np.random.default_rng(6)
    with open(src, "wb") as f:
        for k, (w, h, sel) in enumerate(all_cases):
            words = R.pack_mask(sel)
            if (w * h) % 32 and k & 1:  # garbage in the last word's unused bits
                words[-1] |= np.uint32((int(rng.integers(1, 1 << 32)) << ((w * h) % 32)) & 0xFFFFFFFF)
            f.write(np.uint32([w, h]).tobytes())
            f.write(words.tobytes())
    r = subprocess.run([exe, str(src), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    raw = np.frombuffer(out.read_bytes(), np.uint32)
    at = 0
    for w, h, sel in all_cases:
        tiles, tsel, nsel, traced = T.counts(sel)
        nw = (tiles + 31) // 32
        assert raw[at:at + 3].tolist() == [nsel, tsel, traced], (w, h)
        assert raw[at + 3:at + 3 + nw].tobytes() == T.tile_bit_words(sel).tobytes(), (w, h)
        at += 3 + nw
    assert at == raw.size
    # the restatement's own shape: 37 x 23 is 5 x 3 tiles, the last column 5 pixels wide, the last row 7 high
    sel = np.zeros((23, 37), bool)
    sel[22, 36] = True
    assert T.tile_mask(sel).shape == (3, 5) and T.counts(sel) == (15, 1, 1, 35)
    assert T.traced_pixels(sel).sum() == 35 and T.traced_pixels(sel)[16:, 32:].all()
