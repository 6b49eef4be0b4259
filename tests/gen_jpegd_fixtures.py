"""Writes tests/golden/jpegd: small baseline JPEG files over the samplings, qualities, Huffman tables and restart
intervals the decoder knows, each with the pixels PIL (libjpeg-turbo) decodes it to, and a SHA256SUMS of their own.
Run once by hand with Pillow 12.2 (`python tests/gen_jpegd_fixtures.py`); never run by a test -- the tests read what is
committed, so the machine they run on needs neither PIL nor this script."""
import hashlib
import io
import os

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpegd")

# name: (width, height, sampling (None: grayscale; 0 4:4:4, 1 4:2:2, 2 4:2:0), quality, content, optimize, restart_marker_blocks)
CASES = {
    "g8x8_q75_smooth": (8, 8, None, 75, "smooth", False, 0),
    "c16x16_444_q95_noise": (16, 16, 0, 95, "noise", False, 0),
    "c17x9_420_q75_noise": (17, 9, 2, 75, "noise", False, 0),
    "c33x31_422_q30_smooth": (33, 31, 1, 30, "smooth", False, 0),
    "c48x40_420_q95_noise_opt": (48, 40, 2, 95, "noise", True, 0),
    "c64x48_420_q95_noise": (64, 48, 2, 95, "noise", False, 0),
    "c64x48_444_q30_smooth_rst1": (64, 48, 0, 30, "smooth", False, 1),
    "c250x130_420_q75_smooth": (250, 130, 2, 75, "smooth", False, 0),
    "c250x130_422_q30_noise": (250, 130, 1, 30, "noise", False, 0),
    "g33x31_q95_noise_rst3": (33, 31, None, 95, "noise", False, 3),
    "c48x40_422_q75_noise_rst7": (48, 40, 1, 75, "noise", False, 7),
    "c3x20_420_q75_noise_narrow": (3, 20, 2, 75, "noise", False, 0),      # chroma plane 2 samples wide: replication
    "c4x9_422_q95_noise_narrow": (4, 9, 1, 95, "noise", False, 0),
    "g250x130_q30_noise_opt": (250, 130, None, 30, "noise", True, 0),
    "c17x9_444_q95_smooth_opt": (17, 9, 0, 95, "smooth", True, 0),
    "c33x31_420_q95_noise_rst3_opt": (33, 31, 2, 95, "noise", True, 3),
}


def picture(width, height, gray, content, seed):
    rng = np.random.default_rng(seed)
    if content == "noise":
        return rng.integers(0, 256, size=(height, width) if gray else (height, width, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:height, 0:width]
    base = (xx * 3 + yy * 2) % 256
    return base.astype(np.uint8) if gray else np.stack([base, (base * 2) % 256, 255 - base], axis=2).astype(np.uint8)


def main():
    os.makedirs(OUT, exist_ok=True)
    pixels, sums = {}, []
    for seed, (name, (w, h, samp, q, content, opt, rst)) in enumerate(sorted(CASES.items())):
        kw = dict(quality=q, optimize=opt)
        if samp is not None:
            kw["subsampling"] = samp
        if rst:
            kw["restart_marker_blocks"] = rst
        buf = io.BytesIO()
        Image.fromarray(picture(w, h, samp is None, content, 100 + seed)).save(buf, format="JPEG", **kw)
        data = buf.getvalue()
        assert len(data) <= 24 * 1024, (name, len(data))
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(data)
        pixels[name] = np.asarray(Image.open(io.BytesIO(data)))
        sums.append("%s  %s.jpg" % (hashlib.sha256(data).hexdigest(), name))
    np.savez_compressed(os.path.join(OUT, "pixels.npz"), **pixels)
    sums.append("%s  pixels.npz" % hashlib.sha256(open(os.path.join(OUT, "pixels.npz"), "rb").read()).hexdigest())
    with open(os.path.join(OUT, "SHA256SUMS"), "w") as f:
        f.write("\n".join(sums) + "\n")


if __name__ == "__main__":
    main()
