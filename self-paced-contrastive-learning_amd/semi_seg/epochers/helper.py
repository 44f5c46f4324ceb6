"""Label generators of ``semi_seg/epochers/helper.py:48-65`` (sklearn LabelEncoder == rank among sorted uniques) and
the seeded per-sample flip the epocher and the hook share (deepclustering2 ``TensorRandomFlip(axis=[1,2],
threshold=0.8)`` under ``FixRandomSeed(seed)``; un-vendored third party, restated by contract -- SURVEY 8c)."""
import random
from typing import List

import torch

from ... import functional as F_hip
from ...contrastyou.losses.kl import KL_div, class2one_hot


def supervised_loss(criterion, logits: torch.Tensor, target: torch.Tensor, num_classes: int, fused: bool = True):
    """the supervised criterion of a training step and the batch's Dice counts (new_epocher.py:268-282) -> (loss, (inter,
    union)), ``target`` the [B,H,W] label map.  ``KL_div`` takes the fused launch (``functional.sup_loss_kl_onehot``; with
    ``fused=False`` the composed path), a criterion with ``from_logits`` (contrastyou/losses/dice.py) its own fused kernels,
    anything else the composed path: softmax, one-hot, criterion, arg-max and Dice counts as separate launches."""
    on_head = logits.is_cuda and logits.shape[1] == num_classes <= 16 and logits.shape[0] <= 1024
    if fused and on_head and isinstance(criterion, KL_div):
        return F_hip.sup_loss_kl_onehot(logits, target, criterion._eps)
    if on_head and hasattr(criterion, "from_logits"):
        loss = criterion.from_logits(logits, target)
        return loss, criterion.last_counts
    onehot_target = class2one_hot(target, num_classes)
    loss = criterion(F_hip.softmax_classes(logits), onehot_target, disable_assert=True)
    with torch.no_grad():
        counts = F_hip.dice_counts(F_hip.argmax_classes(logits.detach()), target, num_classes)
    return loss, counts


def begin_epoch(criterion, cur_epoch: int):
    """tell a criterion with an epoch schedule (``BoundaryLoss``: its alpha) which epoch a training epocher runs.  Only the
    criterion's CLASS is asked for ``set_epoch``: for any other criterion nothing of the instance is looked up or changed."""
    if hasattr(type(criterion), "set_epoch"):
        criterion.set_epoch(cur_epoch)


def _label_encode(items):
    index = {v: i for i, v in enumerate(sorted(set(items)))}
    return [index[v] for v in items]


class PartitionLabelGenerator:
    def __call__(self, partition_list: List[str], **kwargs):
        return _label_encode(list(partition_list))


class PatientLabelGenerator:
    def __call__(self, patient_list: List[str], **kwargs):
        return _label_encode(list(patient_list))


class ACDCCycleGenerator:
    def __call__(self, experiment_list: List[str], **kwargs):
        return [0 if e == "00" else 1 for e in experiment_list]


class SIMCLRGenerator:
    def __call__(self, partition_list: List[str], **kwargs):
        return list(range(len(partition_list)))


class FixRandomSeed:
    """Context manager: seed python's and numpy's RNGs, restore their states on exit (contract of
    deepclustering2.FixRandomSeed as used at semi_seg/epochers/new_pretrain.py:57,64 and semi_seg/hooks/infonce.py:177,
    211-214 -- the dense hook draws its points with ``np.random.choice``)."""

    def __init__(self, seed):
        self._seed = seed

    def __enter__(self):
        import numpy as np
        self._state, self._np_state = random.getstate(), np.random.get_state()
        random.seed(self._seed)
        np.random.seed(self._seed % (2 ** 32))
        return self

    def __exit__(self, *a):
        import numpy as np
        random.setstate(self._state)
        np.random.set_state(self._np_state)


class FixAllSeed:
    """Context manager: seed python's, numpy's and torch's CPU generators, restore the three states on exit -- what the mix-up
    hook draws under (``contrastyou.utils.fix_all_seed_within_context`` at semi_seg/hooks/mixup.py:69: ``np.random.beta``, then
    ``torch.randperm`` on the CPU generator).  The reference also reseeds and restores the device generators and sets
    ``PYTHONHASHSEED``: nothing inside this project's uses of the context draws from a device generator, so leaving them alone
    gives the same draws and the same state afterwards; the environment variable is a side effect this mirror does not copy."""

    def __init__(self, seed):
        self._seed = seed

    def __enter__(self):
        import numpy as np
        self._state, self._np_state, self._torch_state = random.getstate(), np.random.get_state(), torch.get_rng_state()
        random.seed(self._seed)
        np.random.seed(self._seed % (2 ** 32))
        torch.default_generator.manual_seed(self._seed)  # (the CPU generator alone; torch.manual_seed seeds the devices' too)
        return self

    def __exit__(self, *a):
        import numpy as np
        random.setstate(self._state)
        np.random.set_state(self._np_state)
        torch.set_rng_state(self._torch_state)


class TensorRandomFlip:
    """Flip a [C,H,W] sample along each of ``axis`` independently when u < threshold (u ~ python ``random``)."""

    def __init__(self, axis=(1, 2), threshold=0.8):
        self._axis = tuple(axis)
        self._threshold = threshold
        self._plans = {}

    def decisions(self, n):
        return [[random.random() < self._threshold for _ in self._axis] for _ in range(n)]

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        dims = [a for a in self._axis if random.random() < self._threshold]
        return x.flip(dims) if dims else x

    def apply_pair(self, first: torch.Tensor, second: torch.Tensor) -> torch.Tensor:
        """``torch.cat([first, stack([self(s) for s in second])])`` (new_pretrain.py:57-58,93) as ONE HIP launch
        (``spcl_flip_pair``) for contiguous [N,C,H,W] GPU tensors of one shape and dtype; draws the same random stream as
        ``apply_batch(second)``."""
        if not (first.is_cuda and second.is_cuda and first.dim() == 4 and first.shape == second.shape
                and first.dtype == second.dtype and tuple(self._axis) == (1, 2)
                and not first.requires_grad and not second.requires_grad):
            return torch.cat([first, self.apply_batch(second)], dim=0)
        from ... import native as _n
        dec = tuple(tuple(d) for d in self.decisions(second.shape[0]))
        key = (dec, second.device, "flags")
        flags = self._plans.get(key)
        if flags is None:
            flags = torch.tensor([int(d[0]) | (int(d[1]) << 1) for d in dec], dtype=torch.uint8, device=second.device)
            if len(self._plans) < 256:
                self._plans[key] = flags
        a, b = first.contiguous(), second.contiguous()
        N, C, H, W = a.shape
        out = torch.empty((2 * N, C, H, W), dtype=a.dtype, device=a.device)
        _n.call("spcl_flip_pair", _n.ptr(a), _n.ptr(b), _n.ptr(out), a.element_size(), N, C, H, W, _n.ptr(flags),
                _n.stream())
        return out

    def apply_batch(self, x: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
        """Batched equivalent of ``stack([self(s) for s in x])`` drawing the same random stream.

        GPU tensors: ONE HIP launch (``spcl_flip_batch``) driven by a per-sample flag byte (bit 0: flip H, bit 1:
        flip W); the flag tensor is cached per decision pattern, so a repeated pattern costs no host->device copy and
        the call can be captured in a hipGraph.  ``out`` (same shape, contiguous) receives the result when given.
        CPU tensors (host-side tests of the random stream only): one gather per flip pattern with torch ops."""
        dec = tuple(tuple(d) for d in self.decisions(x.shape[0]))
        if x.is_cuda:
            if x.dim() != 4 or tuple(self._axis) != (1, 2):
                raise NotImplementedError("the HIP flip handles [N,C,H,W] batches flipped along H and/or W")
            from ... import native as _n
            key = (dec, x.device, "flags")
            flags = self._plans.get(key)
            if flags is None:
                flags = torch.tensor([int(d[0]) | (int(d[1]) << 1) for d in dec], dtype=torch.uint8, device=x.device)
                if len(self._plans) < 256:
                    self._plans[key] = flags
            if x.requires_grad and out is None:  # features on the autograd graph (the dense hook): differentiable form
                from ... import functional as _F
                return _F.flip_batch(x, flags)
            xc = x.contiguous()
            if out is None:
                out = torch.empty_like(xc)
            elif out.shape != xc.shape or not out.is_contiguous() or out.dtype != xc.dtype:
                raise ValueError("apply_batch: `out` must be a contiguous tensor of x's shape and dtype")
            N, C, H, W = xc.shape
            _n.call("spcl_flip_batch", _n.ptr(xc), _n.ptr(out), xc.element_size(), N, C, H, W, _n.ptr(flags),
                    _n.stream())
            return out
        key = (dec, x.device)
        plan = self._plans.get(key)
        if plan is None:
            groups = {}
            for i, d in enumerate(dec):
                groups.setdefault(d, []).append(i)
            plan = [([a + 1 for a, f in zip(self._axis, pat) if f],
                     torch.tensor(idx, dtype=torch.long, device=x.device)) for pat, idx in groups.items() if any(pat)]
            if len(self._plans) < 256:
                self._plans[key] = plan
        res = x.clone() if out is None else out.copy_(x)
        for dims, idx in plan:
            res.index_copy_(0, idx, x.index_select(0, idx).flip(dims))
        return res


def _write_pngs(maps: torch.Tensor, folder: str, filenames):
    """[B,H,W] -> ``folder/<name>.png`` as 8-bit grey (values cast to uint8 as numpy's ``astype`` does); one read-back"""
    import os

    from PIL import Image
    assert maps.dim() == 3 and len(filenames) == maps.shape[0], (tuple(maps.shape), len(filenames))
    arr = maps.detach().to(torch.uint8).cpu().numpy()
    for a, f in zip(arr, filenames):
        path = os.path.join(folder, f + ".png")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(a, mode="L").save(path)


def write_predict(predict_logit: torch.Tensor, save_dir: str, filenames, folder: str = "pred"):
    """``write_predict`` (semi_seg/epochers/helper.py:78-85): the arg-max map of every sample to ``save_dir/pred``.  A
    [B,K,H,W] class map is reduced with the HIP arg-max; a [B,H,W] integer map is taken as the arg-max already formed.
    ``folder`` names another sub-folder of ``save_dir`` (the post-processed maps go to ``pred_lcc``)."""
    import os
    if isinstance(filenames, str):
        filenames = [filenames]
    if predict_logit.dim() == 4:
        from ... import functional as F_hip
        predict_logit = F_hip.argmax_classes(predict_logit)
    assert predict_logit.dim() == 3 and not predict_logit.is_floating_point(), predict_logit.shape
    _write_pngs(predict_logit, os.path.join(save_dir, folder), list(filenames))


def write_uncertainty(entropy: torch.Tensor, save_dir: str, filenames, folder: str = "uncertainty_tta"):
    """a [B,H,W] map of normalised entropies in [0, 1] to ``save_dir/folder`` as ``round(255 * entropy)``, one 8-bit PNG per
    sample (not in the reference: the uncertainty map of the test-time-augmented prediction)"""
    import os
    if isinstance(filenames, str):
        filenames = [filenames]
    assert entropy.dim() == 3 and entropy.is_floating_point(), (tuple(entropy.shape), entropy.dtype)
    _write_pngs((entropy * 255).round().clamp(0, 255), os.path.join(save_dir, folder), list(filenames))


def write_img_target(image: torch.Tensor, target: torch.Tensor, save_dir: str, filenames):
    """``write_img_target`` (semi_seg/epochers/helper.py:88-97): ``image * 255`` to ``save_dir/img`` and the label map to
    ``save_dir/gt``, one PNG per sample ([B,1,H,W] or [B,H,W] tensors)"""
    import os
    if isinstance(filenames, str):
        filenames = [filenames]
    image = image.squeeze(1) if image.dim() == 4 else image
    target = target.squeeze(1) if target.dim() == 4 else target
    assert image.shape == target.shape, (tuple(image.shape), tuple(target.shape))
    _write_pngs(image * 255, os.path.join(save_dir, "img"), list(filenames))
    _write_pngs(target, os.path.join(save_dir, "gt"), list(filenames))
