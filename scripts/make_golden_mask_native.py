"""Writes tests/golden/mask_native.npz from the UNMODIFIED reference's process_mask_native (utils/segment/general.py:54-76), imported
read-only through oracle.ref_shim on torch-CPU.  Needs the reference checkout; no test runs this.

    python scripts/make_golden_mask_native.py

Per case of tests/mask_native_ref.CASES and prototype dtype ("f32"; "f16" = float16 prototypes widened to float32, what the reference's
`protos.float()` sees): {name}_{dtype} = np.packbits of the (n, h0, w0) result, {name}_{dtype}_shape its shape."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import mask_native_ref as mr  # noqa: E402


def main():
    ns = ref_shim.load()
    out = {}
    for name in mr.CASES:
        for pd in mr.PROTO_DTYPES:
            protos, coef, boxes, shape = mr.inputs(name, pd)
            t = [torch.from_numpy(a.astype(np.float32)) for a in (protos, coef, boxes)]
            m = ns.seg_general.process_mask_native(*t, shape)
            assert m.dtype == torch.float32 and tuple(m.shape) == (mr.N,) + tuple(shape)
            top, left, bottom, right = mr.window(protos.shape[1], protos.shape[2], shape)
            assert (bottom - top, right - left) == mr.CASES[name][5:], (name, bottom - top, right - left)
            bits = m.numpy().astype(bool)
            out[f"{name}_{pd}"] = np.packbits(bits)
            out[f"{name}_{pd}_shape"] = np.array(bits.shape, np.int64)
            print(name, pd, bits.shape, "window", (bottom - top, right - left), "set", int(bits.sum()), "per instance", bits.sum((1, 2)).tolist())
    path = os.path.join(ROOT, "tests", "golden", "mask_native.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
