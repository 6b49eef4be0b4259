"""Seeded test pictures for the JPEG encoder's tests (tests/test_jpeg_host.py, tests/test_gpu_jpeg.py): (H, W, 3) uint8
RGB arrays of four kinds -- noise (long codes, every coefficient busy, 0xFF bytes in the stream), constant (DC only),
two-level (samples at 0 and 255: the DCT's largest magnitudes) and a sparse three-colour arrow picture like the ones
the renderer draws (black, blue dots, red lines: long zero runs, EOB everywhere)."""
import numpy as np

import refpics

KINDS = ("noise", "constant", "two_level", "arrows")
QUALITIES = (1, 10, 30, 50, 75, 95, 100)
DISC = [(dx, dy) for dy in range(-2, 3) for dx in range(-2, 3) if dx * dx + dy * dy <= 4]


def picture(kind, W, H, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "constant":
        return np.full((H, W, 3), rng.integers(0, 256, 3, dtype=np.uint8), np.uint8)
    if kind == "two_level":
        return (rng.integers(0, 2, (H, W, 3), dtype=np.uint8) * 255).astype(np.uint8)
    if kind == "arrows":
        img = np.zeros((H, W, 3), np.uint8)
        for y in range(0, H, 4):
            for x in range(0, W, 4):
                if rng.random() < 0.06:
                    for dx, dy in DISC:
                        if 0 <= x + dx < W and 0 <= y + dy < H:
                            img[y + dy, x + dx] = (0, 0, 255)
                    refpics.cv_line(img, x, y, x + int(rng.integers(-12, 13)), y + int(rng.integers(-12, 13)), (255, 0, 0))
        return img
    raise ValueError(kind)


def ragged_cases():
    """256 (W, H, kind, quality, seed): every residue of W mod 16 with every residue of H mod 16, sizes in 1..80 x 1..60."""
    rng = np.random.default_rng(20)
    out = []
    for rw in range(16):
        for rh in range(16):
            n = len(out)
            W = rw + 1 + 16 * int(rng.integers(0, 4 if rw < 15 else 5))
            H = rh + 1 + 16 * int(rng.integers(0, 3 if rh > 11 else 4))
            out.append((min(W, 80), min(H, 60), KINDS[n % 4], QUALITIES[(n // 4) % 7], 1000 + n))
    return out
