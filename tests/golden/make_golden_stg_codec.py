#!/usr/bin/env python
"""Golden vectors for the SPACETIME file codec: the reference's own ``STGPngCompression(use_sort=False)``
(gsplat/compression/stg_compression.py:16-143) compresses and decompresses seeded splats on the CPU, run in the build container
through an in-memory stand-in for ``imageio``; inputs, every plane, meta.json and every decompressed tensor are recorded.
tests/test_gpu_stg_codec.py requires ``STGPngCompression`` here to write the same planes byte for byte and to decode them bit for
bit; tests/test_stg_codec_cpu.py pins the numpy restatement of the decode (tests/stg_codec_reference.py) against the same file.

Two cases, 292 splats each (the reference crops to 289 = 17 x 17):
  stg  all eleven attributes of the STG map plus one extra [n, 2] attribute (-> .npz)
  sh   no colors / features_dir / features_time, but sh0 [n, 1, 3] and shN [n, 15, 3] (-> .npz: the STG map does not list them)
Every channel is a seeded normal / uniform draw -- none constant: maxs == mins is 0 / 0 in the reference.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stg_codec.py
"""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.modules["_gridencoder"] = types.ModuleType("_gridencoder")
STORE = {}
fake = types.ModuleType("imageio.v2")
fake.imwrite = lambda path, img: STORE.__setitem__(os.path.basename(path), np.array(img, copy=True))
fake.imread = lambda path: STORE[os.path.basename(path)]
pkg = types.ModuleType("imageio")
pkg.v2 = fake
sys.modules["imageio"] = pkg
sys.modules["imageio.v2"] = fake
sys.path.insert(0, "/root/reference")
sys.path.insert(0, REPO)

from gsplat.compression.stg_compression import STGPngCompression  # noqa: E402

N = 292


def make_inputs(case: str, rng) -> dict:
    f = lambda a: torch.from_numpy(a.astype(np.float32))  # noqa: E731
    s = {
        "means": f(rng.normal(0, 4.0, (N, 3))),
        "scales": f(rng.uniform(-9, 1, (N, 3))),
        "quats": f(rng.normal(0, 1, (N, 4))),  # NOT normalised: compress() does that
        "opacities": f(rng.normal(0, 3, (N,))),
        "trbf_center": f(rng.uniform(0, 1, (N, 1))),
        "trbf_scale": f(rng.normal(-1, 0.5, (N, 1))),
        "motion": f(rng.normal(0, 0.02, (N, 9))),
        "omega": f(rng.normal(0, 0.1, (N, 4))),
    }
    if case == "stg":
        s["colors"] = f(rng.uniform(0, 1, (N, 3)))
        s["features_dir"] = f(rng.normal(0, 0.3, (N, 3)))
        s["features_time"] = f(rng.normal(0, 0.3, (N, 3)))
        s["extra"] = f(rng.normal(0, 1, (N, 2)))
    else:
        s["sh0"] = f(rng.normal(0, 1, (N, 1, 3)))
        s["shN"] = f(np.round(rng.normal(0, 0.1, (N, 15, 3)) * 16) / 16)  # (an .npz pass-through: coarse values keep the file small)
    return s


def main():
    out = {}
    for case, seed in (("stg", 20), ("sh", 21)):
        STORE.clear()
        splats = make_inputs(case, np.random.default_rng(seed))
        for k, v in splats.items():
            out[f"{case}.input.{k}"] = v.numpy().copy()
        comp = STGPngCompression(use_sort=False, verbose=False)
        with tempfile.TemporaryDirectory() as d:
            comp.compress(d, {k: v.clone() for k, v in splats.items()})
            with open(os.path.join(d, "meta.json")) as f:
                meta_text = f.read()
            dec = comp.decompress(d)
        meta = json.loads(meta_text)
        out[f"{case}.meta"] = np.array(meta_text)
        for fn, img in STORE.items():
            assert img.dtype == np.uint8
            out[f"{case}.plane.{fn}"] = img
        for k, v in dec.items():
            assert torch.is_tensor(v), k
            out[f"{case}.decoded.{k}"] = v.numpy()
        print(f"{case}: {len(dec['means'])} splats, {len(STORE)} planes "
              f"{sorted((fn, img.shape) for fn, img in STORE.items())}; meta keys "
              f"{ {k: sorted(set(m) - {'shape', 'dtype'}) for k, m in meta.items()} }")
    path = os.path.join(HERE, "stg_codec.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
