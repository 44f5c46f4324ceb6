#!/usr/bin/env python3
"""Generate tests/golden/g14_prostate_resize.npz: small u8 label maps and what ``Image.resize(.., NEAREST)`` -- the resize
the reference's wrapper applies to a target under ``Resize(224)`` -- makes of them.  PIL alone writes the expected outputs
(nothing of the project or of the reference is imported), so the fixture pins `spcl_resize_nearest_pil` and
``nearest_resize_table`` to the library itself; ``pil_version`` records which one (a drift shows as with g10).

    python tools/gen_golden_prostate.py            # writes tests/golden/g14_prostate_resize.npz

Keys: ``label{k}`` [H, W] u8, ``resized{k}`` [oh, ow] u8, ``shapes`` [n, 4] = (H, W, oh, ow), ``pil_version``.
(Image resizes -- BILINEAR -- are in g10_augment_recipes.npz.)"""
import os

import numpy as np
import PIL
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "g14_prostate_resize.npz")


def blobs(h, w, classes, seed):
    """smooth class regions: the arg-max of `classes` coarse random fields, enlarged (the shape of a segmentation mask)"""
    rs = np.random.RandomState(seed)
    coarse = rs.rand(classes, max(2, h // 16 + 1), max(2, w // 16 + 1)).astype(np.float32)
    fields = [np.asarray(Image.fromarray(c, "F").resize((w, h), Image.BICUBIC)) for c in coarse]
    return np.argmax(np.stack(fields), axis=0).astype(np.uint8)


def shorter_edge(hw, size):
    """torchvision ``Resize(int)``"""
    h, w = hw
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


def main():
    rs = np.random.RandomState(14)
    cases = [  # (label map, size of the shorter edge)
        (blobs(97, 130, 4, 1), 50),      # -> 50 x 67: an output width that is no multiple of 4
        (blobs(64, 64, 2, 2), 224),      # upscaling: repeated source indices
        (blobs(240, 240, 4, 3), 224),    # a non-integer ratio
        (blobs(256, 320, 2, 4), 224),    # -> 224 x 280
        (blobs(320, 256, 4, 5), 224),    # -> 280 x 224
        (rs.randint(0, 4, size=(240, 240)).astype(np.uint8), 224),  # per-pixel random: every index counts
        (np.array([[3]], dtype=np.uint8), 3),                       # 1 x 1 -> 3 x 3
    ]
    out, shapes = {}, []
    for k, (lab, size) in enumerate(cases):
        oh, ow = shorter_edge(lab.shape, size)
        out[f"label{k}"] = lab
        out[f"resized{k}"] = np.asarray(Image.fromarray(lab, "L").resize((ow, oh), Image.NEAREST))
        shapes.append((*lab.shape, oh, ow))
    np.savez_compressed(OUT, shapes=np.asarray(shapes, dtype=np.int64), pil_version=np.asarray(PIL.__version__), **out)
    print(OUT, os.path.getsize(OUT), "bytes", PIL.__version__)


if __name__ == "__main__":
    main()
