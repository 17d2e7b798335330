#!/usr/bin/env python
"""Golden vectors for the one-bit hash-table files of the Gaussian ANS route, produced by RUNNING THE REFERENCE's
gsplat/compression/entropy_coding_compression.py functions ``to_bin_stream`` / ``from_bin_stream`` on the CPU in the build
container, for seeded +-1 tensors of 8, 13 and 1000 entries.  Only arrays are stored: the signs handed in, the bytes of the file
the reference wrote, and what it read back (13 and 1000 entries also from a file cut short by one byte: the missing bits read as
0, that is -1).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gauss_ans.py
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.modules["_gridencoder"] = types.ModuleType("_gridencoder")
sys.path.insert(0, "/root/reference")

import gsplat.compression.entropy_coding_compression as E  # noqa: E402


def main():
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for n in (8, 13, 1000):
            g = torch.Generator().manual_seed(100 + n)
            signs = (torch.randint(0, 2, (n,), generator=g) * 2 - 1).to(torch.float32)
            path = os.path.join(d, f"{n}.bin")
            E.to_bin_stream(signs, path)
            data = np.fromfile(path, dtype=np.uint8)
            back = E.from_bin_stream(path, n).numpy()
            assert back.dtype == np.float32 and np.array_equal(back, signs.numpy()) and data.size == (n + 7) // 8
            out[f"signs.{n}"] = signs.numpy()
            out[f"bytes.{n}"] = data
            out[f"back.{n}"] = back
            if n > 8:
                data[:-1].tofile(path)
                out[f"back_short.{n}"] = E.from_bin_stream(path, n).numpy()
            print(f"{n} entries: {data.size} bytes, {int((signs > 0).sum())} positive")
    path = os.path.join(HERE, "gauss_ans.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
