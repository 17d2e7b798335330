#!/usr/bin/env python
"""Pinned bytes of the two ANS containers: the inputs and the whole ``.bin`` file of small cases, written by this project's own
numpy coders (``ans_reference`` and ``gauss_ans_reference``, the definitions of the two formats) AS THEY STOOD AT COMMIT 54cf377
("Hash-grid Gaussian rANS codec on HIP: the _gaussian_ans file pair"), the last one at which each module carried its own copy of
the stream machinery.  The GPU tests compare the HIP coders with the numpy ones, so a change that moved both the same way would
pass them; these arrays do not move.  Only the two ``*_reference`` modules do any coding here; the inputs are the tests' own
(``ans_cases.draw``, ``gauss_ans_cases.model_case``).

Factorized (``f.<N>.<P>.*``):  S = 5, C = 3 (one channel of each distribution of ``ans_cases``), N in 1, 4, 5, 6, 17, P in 8, 12, 14.
Gaussian (``g.<name>.*``):     S = 5, C = 2 with ``model_case`` at the same N; ``freq1``: mu_q = 2040, k = 0 and symbols below
40, so that every symbol has frequency 1 and every full stream fills its worst case of 2 S + S // 512 bytes; ``long``: S = 1024,
N = 1025.

Regenerating the file from a later commit defeats its purpose: do so only for a deliberate change of a format.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ans_containers.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

from ans_cases import DISTRIBUTIONS, draw, probabilities  # noqa: E402
from gauss_ans_cases import model_case  # noqa: E402
from gscodec_studio_amd.compression import ans_reference as A  # noqa: E402
from gscodec_studio_amd.compression import gauss_ans_reference as G  # noqa: E402

SIZES = (1, 4, 5, 6, 17)
S = 5


def main():
    out = {}
    for n in SIZES:
        sym = np.concatenate([draw(kind, n, 1) for kind in DISTRIBUTIONS], axis=1)
        prob = probabilities(sym)
        out[f"f.{n}.sym"], out[f"f.{n}.prob"] = sym, prob
        for bits in (8, 12, 14):
            blob = A.encode(sym, prob, stream_len=S, bits=bits)
            assert np.array_equal(A.decode(blob, prob), sym)
            out[f"f.{n}.{bits}.blob"] = blob
    cases = {str(n): (S,) + model_case(n, 2, 700 + n) for n in SIZES}
    low = np.random.default_rng(11).integers(0, 40, (17, 2)).astype(np.uint8)
    cases["freq1"] = (S, low, np.full((17, 2), G.MU_Q_MAX, np.int16), np.zeros((17, 2), np.uint8))
    cases["long"] = (1024,) + model_case(1025, 2, 1025)
    for name, (s_len, sym, mu_q, k) in cases.items():
        blob = G.encode(sym, mu_q, k, stream_len=s_len)
        assert np.array_equal(G.decode(blob, mu_q, k), sym)
        out[f"g.{name}.stream_len"] = np.int64(s_len)
        out[f"g.{name}.sym"], out[f"g.{name}.mu_q"], out[f"g.{name}.k"], out[f"g.{name}.blob"] = sym, mu_q, k, blob
    sizes = np.diff(G.parse_container(out["g.freq1.blob"])[3]) - 4
    assert np.all(sizes[[0, 1, 2, 4, 5, 6]] == 2 * S + S // 512), sizes  # the full streams meet the bound
    path = os.path.join(HERE, "ans_containers.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
