"""Writes tests/golden/quad.npz from the UNMODIFIED reference's `LoadImagesAndLabels.collate_fn4` (utils/dataloaders.py:865-891), imported
read-only through oracle.ref_shim on torch-CPU and called on seeded inputs.  Needs the reference checkout; no test runs this.

    python scripts/make_golden_quad.py

Stored: data only.  `imgs8` (8, 3, 32, 32) uint8 and `targets8` (nt, 6) float32 as `collate_fn` yields them (image index in column 0; 0, 1 and
several rows per image, the second group of four without any), `imgs11` / `targets11` for the batch of 11 (three samples dropped), `seeds`
and per seed s: flags{s} (the coins `random.seed(s)` makes the reference draw), img{s}, lab{s}; for the batch of 11: seed11, img11, lab11,
npaths11.  The script ASSERTS that the seeds cover the two mixed orders of the coins, both-upsampled and both-tiled."""
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import quad_ref as qr  # noqa: E402

H = W = 32


def inputs(B, counts, seed):
    """-> (imgs (B, 3, H, W) uint8, targets (nt, 6) float32 in collate_fn's layout)."""
    rng = np.random.default_rng(seed)
    imgs = qr.byte_patterns(B, 3, H, W, seed)
    rows = []
    for b, k in enumerate(counts):
        lb = np.zeros((k, 6), np.float32)
        lb[:, 0] = b
        lb[:, 1] = rng.integers(0, 80, k)
        lb[:, 2:4] = rng.uniform(0.05, 0.95, (k, 2))
        lb[:, 4:6] = rng.uniform(0.02, 0.6, (k, 2))
        rows.append(lb)
    return imgs, np.concatenate(rows, 0).astype(np.float32)


def reference(dl, imgs, targets, seed):
    """The reference's collate_fn4 on the samples `collate_fn` would have been given, coins from random.seed(seed)."""
    t = torch.from_numpy(targets)
    batch = [(torch.from_numpy(imgs[b]), t[t[:, 0] == b].clone(), f"img{b}", (b, b)) for b in range(len(imgs))]
    random.seed(seed)
    flags = [random.random() < 0.5 for _ in range(len(imgs) // 4)]
    random.seed(seed)
    im4, lab4, path4, shapes4 = dl.LoadImagesAndLabels.collate_fn4(batch)
    assert im4.dtype == torch.uint8 and lab4.dtype == torch.float32
    return flags, im4.numpy(), lab4.numpy(), list(path4), list(shapes4)


def main():
    ref_shim.load()
    cwd = os.getcwd()
    os.chdir(ref_shim.REFERENCE_ROOT)
    try:
        import utils.dataloaders as dl
    finally:
        os.chdir(cwd)
    imgs8, targets8 = inputs(8, [0, 1, 3, 2, 0, 0, 0, 0], 1)
    out = {"imgs8": imgs8, "targets8": targets8}
    want = {(True, False): None, (False, True): None, (True, True): None, (False, False): None}
    for seed in range(100):
        random.seed(seed)
        fl = tuple(random.random() < 0.5 for _ in range(2))
        if want[fl] is None:
            want[fl] = seed
    seeds = sorted(want.values())
    assert None not in want.values()
    for seed in seeds:
        flags, im4, lab4, _, _ = reference(dl, imgs8, targets8, seed)
        assert im4.shape == (2, 3, 2 * H, 2 * W)
        assert np.array_equal(im4, qr.collate4_images(imgs8, flags)) and np.array_equal(lab4, qr.collate4_labels(targets8, flags))
        out[f"flags{seed}"], out[f"img{seed}"], out[f"lab{seed}"] = np.array(flags), im4, lab4
    imgs11, targets11 = inputs(11, [2, 0, 1, 3, 1, 1, 0, 2, 1, 2, 0], 2)
    s11 = want[(False, True)]
    flags, im4, lab4, path4, shapes4 = reference(dl, imgs11, targets11, s11)
    assert im4.shape[0] == 2 and path4 == ["img0", "img1"] and shapes4 == [(0, 0), (1, 1)] and len(lab4) == 2 + 0 + 1 + 3 + 1
    out.update(imgs11=imgs11, targets11=targets11, seed11=np.array(s11), flags11=np.array(flags), img11=im4, lab11=lab4, npaths11=np.array(len(path4)))
    out["seeds"] = np.array(seeds)
    path = os.path.join(ROOT, "tests", "golden", "quad.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), {tuple(k): v for k, v in want.items()})


if __name__ == "__main__":
    main()
