"""Seeded image builders and the case list of the SIFT detector's edge tests (tests/test_sift_edges_cpu.py checks that the cases are fit
for purpose with the restatement alone, tests/test_sift_edges_gpu.py runs them on the device).  No GPU and no files."""
import numpy as np


def blocks(h, w, seed, k=4):
    """Uniform random bytes on a k x k block grid, cropped to h x w: doubled by INTER_LINEAR it has plateaus (exact ties), and it is
    rich in keypoints."""
    r = np.random.default_rng(seed)
    g = r.integers(0, 256, ((h + k - 1) // k, (w + k - 1) // k), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(g, np.ones((k, k), np.uint8))[:h, :w])


def noise(h, w, seed, channels=1):
    """Independent uniform bytes; channels = 3 gives [h, w, 3] (BGR), which goes through BGR-to-gray."""
    r = np.random.default_rng(seed)
    return r.integers(0, 256, (h, w) if channels == 1 else (h, w, channels), dtype=np.uint8)


def constant(h, w, value, channels=1):
    return np.full((h, w) if channels == 1 else (h, w, channels), value, np.uint8)


def blob(h, w, cx, cy, s):
    """An isotropic Gaussian blob of standard deviation s centred on (cx, cy), on a gray background."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.clip(np.rint(60 + 150 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))), 0, 255).astype(np.uint8)


def checkerboard(h, w, k=8, lo=40, hi=215):
    """A k-pixel checkerboard: every extremum is tied with its mirror images."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((yy // k) + (xx // k)) % 2 == 0, lo, hi).astype(np.uint8)


# (h, w, seed of blocks(h, w, seed)): what the size is for.  The seeds are chosen so that the restatement's fragile share stays under the
# cap of tests/test_sift_edges_cpu.py.
BLOCK_SIZES = [
    (2, 2, 1),           # the smallest legal size: one 4 x 4 octave, every blur radius larger than the level
    (2, 300, 1),         # one octave, 4 rows: no interior
    (2, 16384, 1),       # the same at the width limit: 512 column tiles
    (3, 200, 1),         # octaves of 6 and 3 rows: no interior, reflection folds several times
    (5, 64, 1),          # 10 rows: ih = 0, exactly no interior
    (6, 200, 5),         # 12 rows: an interior two rows high; octave 1 has 6 rows
    (8, 32, 1),          # doubled 16 x 64: exactly one blur tile
    (9, 33, 5),          # 18 x 66: one tile plus two pixels each way, odd at every halving
    (31, 33, 2),         # tile seams in octaves 0 and 1, one pixel either side
    (32, 32, 1),
    (64, 64, 4),
    (33, 65, 3),
    (63, 129, 2),
    (65, 127, 2),
    (16, 513, 2),        # 1026 columns: seam plus two
    (12, 16384, 1),      # the size limit in each direction, four octaves
    (16384, 12, 1),
    (128, 257, 2),       # about 950 keypoints, in pyramid octaves 0 to 3
]
NOISE_SIZES = [(33, 65, 2), (65, 127, 3), (128, 257, 4)]       # 3 channels: BGR-to-gray at odd sizes
# blocks of 4 are constant down a column of 2 or 3 rows, so a wrong fold of the row index would not show: gray noise at the thin sizes
THIN_NOISE_SIZES = [(2, 2, 5), (2, 300, 6), (2, 16384, 7), (3, 200, 8), (5, 64, 9), (6, 200, 20)]
FLAT = (40, 56)          # the size of the images without keypoints, and of the mixed batch

CASES = [(f"blocks_{h}x{w}", blocks(h, w, s)) for h, w, s in BLOCK_SIZES] + \
        [(f"noise3_{h}x{w}", noise(h, w, s, 3)) for h, w, s in NOISE_SIZES] + \
        [(f"noise_{h}x{w}", noise(h, w, s)) for h, w, s in THIN_NOISE_SIZES] + \
        [("const_gray_40x56", constant(*FLAT, 93)), ("zero_bgr_40x56", constant(*FLAT, 0, 3))]

# the cases in which nothing may be found: no octave with an interior, or no texture
EMPTY = ["blocks_2x2", "blocks_2x300", "blocks_2x16384", "blocks_3x200", "blocks_5x64", "const_gray_40x56", "zero_bgr_40x56",
         "noise_2x2", "noise_2x300", "noise_2x16384", "noise_3x200", "noise_5x64"]

BATCH_GRAY = (33, 65)    # three different images of one size through one call
BATCH_COLOUR = (63, 129)
TIE_SIZE = (64, 80)      # blocks(k=8) and the 8-pixel checkerboard


def batch_gray():
    return np.stack([blocks(*BATCH_GRAY, 21), noise(*BATCH_GRAY, 22), blocks(*BATCH_GRAY, 23, k=3)])


def batch_colour():
    return np.stack([noise(*BATCH_COLOUR, 31, 3), np.repeat(blocks(*BATCH_COLOUR, 32)[..., None], 3, 2), noise(*BATCH_COLOUR, 33, 3)])


def mixed_batch(colour=False):
    """[blocks, constant, blocks', zero] at FLAT; the colour form gives every image three (different) channels where it has texture."""
    a, b = blocks(*FLAT, 41), blocks(*FLAT, 42)
    if not colour:
        return np.stack([a, constant(*FLAT, 93), b, constant(*FLAT, 0)])
    col = lambda g, s: np.stack([g, np.roll(g, 1, 1), blocks(*FLAT, s)], 2)
    return np.stack([col(a, 43), constant(*FLAT, 93, 3), col(b, 44), constant(*FLAT, 0, 3)])


def tie_images():
    return [("blocks8", blocks(*TIE_SIZE, 52, k=8)), ("checker8", checkerboard(*TIE_SIZE, 8))]


_REF = {}


def reference(name, img):
    """The restatement's (Gaussian levels, DoG levels, keypoints, seconds) for a named image, computed once per process and left unchanged."""
    if name not in _REF:
        import time
        from tests import sift_ref as R
        t = time.perf_counter()
        gp, dp = R.pyramid(img)
        det = R.detect_from_pyramid(gp, dp)
        _REF[name] = (gp, dp, det, time.perf_counter() - t)
    return _REF[name]
