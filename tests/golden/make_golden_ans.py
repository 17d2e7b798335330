#!/usr/bin/env python
"""Golden vectors for the factorized ANS codec, produced by RUNNING THE REFERENCE's
gsplat/compression/entropy_coding_compression.py functions ``_compress_factorized_ans`` / ``_decompress_factorized_ans`` in the
build container.  ``constriction`` is not installed; the two functions use it only as a lossless container for the symbols, so a
stand-in module is registered for the duration of this script that RECORDS what the coder is handed (the messages, in stack
order, and the probabilities of the categorical models) and hands it back on decode.  What is recorded -- the symbols, the
``_prob.npy`` table and the decoded parameters -- is the reference's own arithmetic.  Only arrays are stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ans.py
"""
import contextlib
import io
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.modules["_gridencoder"] = types.ModuleType("_gridencoder")

STACKS = {}  # token -> list of (message, probabilities) in the order encode_reverse was called


class Categorical:
    def __init__(self, probabilities, perfect=True):
        self.probabilities = np.array(probabilities, copy=True)


class AnsCoder:
    def __init__(self, compressed=None):
        self.stack = [] if compressed is None else list(STACKS[int(compressed[0])])

    def encode_reverse(self, message, model):
        self.stack.append((np.array(message, copy=True), model.probabilities))

    def get_compressed(self):
        token = len(STACKS) + 1
        STACKS[token] = list(self.stack)
        return np.array([token], dtype=np.uint32)

    def decode(self, model, amount):
        message, probabilities = self.stack.pop()  # a stack: the last message pushed is the first one out
        assert len(message) == amount and np.array_equal(probabilities, model.probabilities)
        return message


constriction = types.ModuleType("constriction")
constriction.stream = types.ModuleType("constriction.stream")
constriction.stream.model = types.ModuleType("constriction.stream.model")
constriction.stream.stack = types.ModuleType("constriction.stream.stack")
constriction.stream.model.Categorical = Categorical
constriction.stream.stack.AnsCoder = AnsCoder
for mod in (constriction, constriction.stream, constriction.stream.model, constriction.stream.stack):
    sys.modules[mod.__name__] = mod
sys.path.insert(0, "/root/reference")

import gsplat.compression.entropy_coding_compression as E  # noqa: E402


def plant(x):
    """Exact .5 ties of the 8-bit quantizer and the channel extremes: with min 0 and max 255 * 2^-5 (both planted) the
    normalised value times 255 is x * 32, so (k + 0.5) / 32 sits exactly between symbols k and k + 1."""
    x = x.copy()
    for c in range(x.shape[1]):
        lo, hi = -3.0 - c, -3.0 - c + 255.0 / 32.0
        x[:, c] = lo + (x[:, c] - x[:, c].min()) / (x[:, c].max() - x[:, c].min()) * (hi - lo)
        x[0, c], x[1, c] = lo, hi
        x[2:8, c] = lo + (np.array([0, 1, 2, 127, 128, 253]) + 0.5) / 32.0
    return x.astype(np.float32)


def main():
    rng = np.random.default_rng(11)
    n = 4096
    quats = rng.normal(0, 1, (n, 4))
    quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    cases = {"scales": plant(rng.normal(-4.5, 1.2, (n, 3))), "quats": quats.astype(np.float32)}
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name, x in cases.items():
            with contextlib.redirect_stdout(io.StringIO()):
                meta = E._compress_factorized_ans(d, name, torch.from_numpy(x), n_sidelen=64)
                decoded = E._decompress_factorized_ans(d, name, meta).numpy()
            token = int(np.fromfile(os.path.join(d, f"{name}.bin"), dtype=np.uint32)[0])
            symbols = np.stack([m for m, _ in reversed(STACKS[token])])  # encode_reverse ran from the last channel to the first
            prob = np.load(os.path.join(d, f"{name}_prob.npy"))
            assert symbols.shape == (x.shape[1], n) and prob.shape == (x.shape[1], 256) and prob.dtype == np.float32
            assert decoded.dtype == np.float32 and decoded.shape == x.shape
            out[f"{name}.x"] = x
            out[f"{name}.mins"] = np.asarray(meta["mins"], np.float32)
            out[f"{name}.maxs"] = np.asarray(meta["maxs"], np.float32)
            out[f"{name}.symbols"] = symbols.astype(np.uint8)  # [C, N], as handed to the coder
            out[f"{name}.prob"] = prob
            out[f"{name}.decoded"] = decoded
            print(f"{name}: symbols {symbols.shape} in [{symbols.min()}, {symbols.max()}], max |decoded - x| = "
                  f"{np.abs(decoded - x).max():.4g}")
    path = os.path.join(HERE, "ans.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
