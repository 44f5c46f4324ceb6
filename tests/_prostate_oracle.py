"""Oracle helpers of the Prostate data seam (tests/test_prostate_host.py, tests/test_gpu_prostate_data.py): PIL's own
``Image.resize`` as the reference for label maps (NEAREST) and images (BILINEAR), the sweep of axis lengths the index table
is checked over, and synthetic labelled Prostate stores.  Test infrastructure; nothing here is product code."""
import os

import numpy as np
import torch
from PIL import Image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_prostate_resize.npz")
SWEEP_IN = range(1, 400)
SWEEP_OUT = (1, 2, 3, 7, 100, 160, 224, 225, 256, 280, 320, 333, 512)  # 399 x 13 = 5187 cases


def g14():
    return np.load(GOLDEN)


def pil_nearest_table(n_in: int, n_out: int):
    """the source index PIL picks for every output pixel of one axis: ``resize(NEAREST)`` of an `I`-mode ramp 0 .. n_in - 1"""
    ramp = Image.fromarray(np.arange(n_in, dtype=np.int32)[None, :].copy(), "I")
    return np.asarray(ramp.resize((n_out, 1), Image.NEAREST))[0].tolist()


def closed_form_table(n_in: int, n_out: int):
    """the tempting restatement ``int((x + 0.5) * scale)``: NOT what PIL computes (it accumulates ``xo += scale``)"""
    scale = n_in / n_out
    return [int((x + 0.5) * scale) for x in range(n_out)]


def pil_resize_nearest(lab_u8, out_hw):
    oh, ow = out_hw
    return np.asarray(Image.fromarray(np.ascontiguousarray(lab_u8), "L").resize((ow, oh), Image.NEAREST))


def pil_resize_bilinear(img_u8, out_hw):
    oh, ow = out_hw
    return np.asarray(Image.fromarray(np.ascontiguousarray(img_u8), "L").resize((ow, oh), Image.BILINEAR))


def prostate_arrays(scans, per_scan=2, size=240, seed=0, classes=2):
    """(stems, images u8 [S, size, size], label maps u8) of a synthetic Prostate set: smooth grey blobs, the label map a
    threshold of the blob plus a few per-pixel flips (so that single label pixels matter)"""
    rs = np.random.RandomState(seed)
    stems, imgs, labs = [], [], []
    for s in scans:
        coarse = rs.rand(max(2, size // 32), max(2, size // 32)).astype(np.float32)
        base = np.asarray(Image.fromarray(coarse, "F").resize((size, size), Image.BICUBIC)).clip(0, 1)
        for k in range(per_scan):
            a = np.clip(base * (0.6 + 0.4 * k / per_scan) + 0.1 * rs.rand(size, size), 0, 1)
            u8 = np.round(a * 255).astype(np.uint8)
            lab = np.minimum(u8.astype(np.int64) * classes // 160, classes - 1).astype(np.uint8)
            flip = rs.rand(size, size) < 0.02
            lab[flip] = (lab[flip] + 1) % classes
            stems.append(f"{s}_{k:02d}")
            imgs.append(u8)
            labs.append(lab)
    return stems, np.stack(imgs), np.stack(labs)


def prostate_store(stems, imgs_u8, labs_u8, device):
    """``ProstateSliceStore`` of 8-bit levels k / 255 with label maps"""
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg.data import ProstateSliceStore
    images = torch.from_numpy(imgs_u8.astype(np.float32) / np.float32(255))
    return ProstateSliceStore(images.to(device), stems, targets=torch.from_numpy(labs_u8).to(device))


def pil_resized_arrays(imgs_u8, labs_u8, out_hw):
    """every slice resized by PIL on the host: `L` BILINEAR, label map NEAREST"""
    return (np.stack([pil_resize_bilinear(a, out_hw) for a in imgs_u8]),
            np.stack([pil_resize_nearest(a, out_hw) for a in labs_u8]))
