"""The JPEG files of the GPU-decode tests (test_jpeg_dec.py on the host, test_jpeg_dec_gpu.py on the
device): a matrix of small files that reaches every branch of the decode, each with its PIL oracle."""
import functools
import io

import numpy as np
from PIL import Image

# H x W: a single MCU at each sampling, one pixel, non-multiples of 8 and 16, odd chroma widths, more than
# one MCU row at 4:2:0 (H >= 33), chroma width <= 2 (the replicate rule: 5x3, 3x5), wide and tall
SIZES = [(16, 16), (8, 8), (1, 1), (17, 13), (33, 47), (24, 40), (9, 31), (40, 24), (5, 3)]


def picture(h: int, w: int, noisy: bool, seed: int = 0) -> np.ndarray:
    if noisy:
        return np.random.default_rng(seed + 1000 * h + w).integers(0, 256, (h, w, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 7 + yy * 3) % 256, 255 - (xx * 2 + yy * 5) % 256, (xx * yy + 31) % 256], -1).astype(np.uint8)


def save(img: np.ndarray, **kw) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def oracle(data: bytes) -> np.ndarray:
    """The expression inside codec/image.py:decode_image."""
    return np.array(Image.open(io.BytesIO(data)).convert("RGB"))


@functools.lru_cache(maxsize=None)
def matrix():
    """[(name, jpeg bytes, oracle array)]: the full cross product of the sizes x subsampling 0 / 1 / 2 x
    quality 30 / 75 / 90 / 100 x smooth / noisy content x {default, optimized Huffman tables, restart marker
    every 3 blocks}, then greyscale files, and one 224x224 and one 480x640 image at q90."""
    out = []
    for h, w in SIZES:
        for ss in (0, 1, 2):
            for q in (30, 75, 90, 100):
                for noisy in (False, True):
                    for kw in ({}, {"optimize": True}, {"restart_marker_blocks": 3}):
                        name = f"{h}x{w}-ss{ss}-q{q}-{'noise' if noisy else 'smooth'}" + "".join(f"-{k}" for k in kw)
                        data = save(picture(h, w, noisy), quality=q, subsampling=ss, **kw)
                        out.append((name, data, oracle(data)))
    for h, w in ((16, 16), (3, 5), (33, 47)):
        buf = io.BytesIO()
        Image.fromarray(picture(h, w, True)[..., 0]).save(buf, format="JPEG", quality=90)
        out.append((f"{h}x{w}-grey", buf.getvalue(), oracle(buf.getvalue())))
    for h, w in ((224, 224), (480, 640)):
        base = picture(h, w, False).astype(np.int32) + np.random.default_rng(h).integers(-20, 20, (h, w, 3))
        data = save(np.clip(base, 0, 255).astype(np.uint8), quality=90)
        out.append((f"{h}x{w}-q90", data, oracle(data)))
    return out
