"""Time the build of a Prostate-shaped labelled store on the device -- ``--slices`` (1500) slices of 320 x 320, images and
label maps, ``Resize(224)`` of both (``DeviceSliceStore.resized``: `spcl_resize_bilinear_pil` + `spcl_resize_nearest_pil`) --
against a host loop of ``Image.resize`` (BILINEAR / NEAREST) over the same slices, and one ``get_data`` call:

* ``kernels``: the two resize calls alone (events around ``--reps`` repetitions), then the label kernel by itself on a
  cache-cold source with its byte rate;
* ``store``: upload + ``resized(224)`` of the whole store, wall clock, against the host loop (+ the upload of its result);
* ``get_data``: ``get_data({"name": "prostate", "labeled_scan_num": 5}, ..)`` on the 320^2 store (the build-time resize
  included) and on a store resized beforehand; and what the ``resized_to`` mark saves: the resize every loader built on an
  unmarked store runs again (five loaders on a pre-train run: labelled, unlabelled, contrastive, validation, test).
  The commit before this one raised ``NotImplementedError`` from this call for either store, so there is no earlier time
  to set beside it.

One process, to be run under a time limit of its own; no pass / fail bar.

    timeout -k 10 600 python tools/diag/prostate_store_time.py [--slices 1500] [--reps 10] [--out profiles/prostate_store_time.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
HW, SIZE = 320, 224


def _events(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps  # ms


def _wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "prostate_store_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prostate_store_time.py measures on the GPU: no device found")
    import spcl_amd  # noqa: F401
    from PIL import Image
    from spcl_amd import native as _n
    from spcl_amd.semi_seg.data import ProstateSliceStore, augment as A, creator as C
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    per_scan = 30
    n_scans = max(50, args.slices // per_scan)
    S = n_scans * per_scan
    rs = np.random.RandomState(0)
    imgs = rs.randint(0, 256, size=(S, HW, HW), dtype=np.uint8)
    labs = rs.randint(0, 2, size=(S, HW, HW), dtype=np.uint8)
    stems = [f"Case{s:02d}_{k:02d}" for s in range(n_scans) for k in range(per_scan)]
    say(f"Prostate-shaped store: {S} slices of {HW} x {HW} ({n_scans} scans), images + label maps -> Resize({SIZE})")

    # ---- the two kernels alone
    d_img = torch.from_numpy(imgs).cuda().float().div_(255.0)
    d_lab = torch.from_numpy(labs).cuda()
    t_bil = _events(lambda: A.resize_store(d_img, SIZE), args.reps)
    t_nn = _events(lambda: A.resize_labels(d_lab, SIZE), args.reps)
    say(f"calls: resize_store (bilinear, f32, two passes + coefficient upload) {t_bil:.2f} ms, resize_labels (nearest, u8, one "
        f"gather + table upload) {t_nn:.3f} ms; {args.reps} reps each on one store (its {S * HW * HW / 1e6:.0f} MB of label maps "
        f"stay in the Infinity Cache between reps)")
    # the label kernel by itself (tables uploaded once), rotating over four stores so that no rep finds its source in the
    # 256 MiB Infinity Cache: 4 x (source + output) = 0.9 GB
    tx = torch.tensor(A.nearest_resize_table(HW, SIZE), dtype=torch.int32).cuda()
    srcs = [d_lab.clone() for _ in range(4)]
    outs = [torch.empty(S, SIZE, SIZE, dtype=torch.uint8, device="cuda") for _ in range(4)]
    turn = [0]

    def one_launch():
        k = turn[0] = (turn[0] + 1) % 4
        _n.call("spcl_resize_nearest_pil", _n.ptr(srcs[k]), S, HW, HW, _n.ptr(tx), _n.ptr(tx), _n.ptr(outs[k]), SIZE, SIZE,
                _n.stream())

    t_k = _events(one_launch, 50 * args.reps, warmup=8)
    read = S * SIZE * HW  # the source rows the gather touches, whole (224 of every 320 rows; every 64-B line of a row is hit)
    say(f"spcl_resize_nearest_pil alone, cache-cold source ({50 * args.reps} launches over four stores): {t_k * 1e3:.1f} us per "
        f"launch = {(S * SIZE * SIZE + read) / t_k / 1e9:.2f} TB/s of bytes it must move ({S * SIZE * SIZE / 1e6:.0f} MB written, "
        f"{read / 1e6:.0f} MB of touched source rows); the measured streaming rate of this chip is about 6.3 TB/s")
    del d_img, d_lab, srcs, outs

    # ---- the whole store: device path against the host loop
    def device_store():
        images = torch.from_numpy(imgs).float().div_(255.0).cuda()
        return ProstateSliceStore(images, stems, targets=torch.from_numpy(labs).cuda()).resized(SIZE)

    def host_store():
        ri = np.stack([np.asarray(Image.fromarray(a, "L").resize((SIZE, SIZE), Image.BILINEAR)) for a in imgs])
        rl = np.stack([np.asarray(Image.fromarray(a, "L").resize((SIZE, SIZE), Image.NEAREST)) for a in labs])
        store = ProstateSliceStore(torch.from_numpy(ri).float().div_(255.0).cuda(), stems, targets=torch.from_numpy(rl).cuda())
        store.resized_to = SIZE
        return store

    device_store()  # (first call: library load, allocator warm-up)
    t_dev, dev = _wall(device_store)
    t_host, host = _wall(host_store)
    same = torch.equal(dev.images, host.images) and torch.equal(dev.targets, host.targets)
    say(f"store: host u8 -> device store resized on the device {t_dev:.0f} ms; host loop of Image.resize over the same slices + "
        f"upload {t_host:.0f} ms; device / host = {t_dev / t_host:.3f}; same bits: {same}")

    # ---- get_data
    raw = ProstateSliceStore(torch.from_numpy(imgs).float().div_(255.0).cuda(), stems, targets=torch.from_numpy(labs).cuda())
    val_stems = [f"Case{s:02d}_{k:02d}" for s in range(n_scans, n_scans + 3) for k in range(per_scan)]

    def val_store(src):
        n = len(val_stems)
        return ProstateSliceStore(src.images[:n].clone(), val_stems, targets=src.targets[:n].clone())

    def get_data(src):
        C.register_dataset("prostate", lambda mode: src if mode == "train" else val_store(src))
        try:
            return C.get_data({"name": "prostate", "labeled_scan_num": 5}, {"batch_size": 4}, {"batch_size": 4})
        finally:
            C._FACTORIES.pop("prostate")

    get_data(host)
    t_raw, _ = _wall(lambda: get_data(raw))
    t_pre, loaders = _wall(lambda: get_data(host))
    lab_set = loaders[0].dataset
    t_again = _events(lambda: A.RecipeViews(raw.images[:len(lab_set)], "prostate_pretrain", (SIZE, SIZE),
                                            labels=raw.targets[:len(lab_set)]), 3, warmup=1)
    t_all = _events(lambda: A.RecipeViews(raw.images, "prostate_pretrain", (SIZE, SIZE)), 3, warmup=1)
    say(f"get_data (labelled 5 scans of {n_scans}, batch 4): on the {HW}^2 store, resize included, {t_raw:.0f} ms; on a store "
        f"resized beforehand {t_pre:.0f} ms (the commit before this one: NotImplementedError for both)")
    say(f"what the resized_to mark saves per loader on an unmarked {HW}^2 store: RecipeViews of the {len(lab_set)} labelled slices with "
        f"label maps {t_again:.1f} ms, of all {S} slices without (the contrastive / unlabelled loader) {t_all:.1f} ms")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        out.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
