"""The ANS bitstream without a GPU: the frequency normaliser, the numpy coder that defines the format
(gscodec_studio_amd/compression/ans_reference.py), the container's validation (host checks; nothing is launched) and the size of
the files against the empirical entropy."""
import io
import os
import struct

import numpy as np
import pytest

from ans_cases import DISTRIBUTIONS, draw, entropy_bytes, probabilities, size_bound
from gscodec_studio_amd.compression import ans_reference as R

S = 1024


@pytest.mark.parametrize("bits", [14, 12, 8])
def test_frequency_normaliser(bits):
    rng = np.random.default_rng(3)
    sym = np.concatenate([draw(k, 5000, 1) for k in DISTRIBUTIONS], axis=1)
    prob = probabilities(sym)
    rare = np.zeros((1, 256), np.float32)  # entries far below 2^-bits, and an exact tie for the largest
    rare[0, [3, 200]] = 0.4999
    rare[0, 10:60] = 1e-7
    heavy = rng.random((1, 256)).astype(np.float32)
    heavy /= heavy.sum() * 0.5  # sums to 2: the surplus has to be taken away again
    prob = np.concatenate([prob, rare, heavy])
    freq = R.normalize_frequencies(prob, bits)
    assert freq.dtype == np.uint32 and freq.shape == prob.shape
    assert np.all(freq.sum(axis=1) == 1 << bits)
    assert np.all(freq[prob > 0] >= 1) and np.all(freq[prob == 0] == 0)
    assert np.array_equal(freq, R.normalize_frequencies(prob.copy(), bits))  # deterministic
    f = io.BytesIO()
    np.save(f, prob)  # what travels in <name>_prob.npy
    f.seek(0)
    assert np.array_equal(freq, R.normalize_frequencies(np.load(f), bits))
    # the difference goes to the largest entry, the lowest index on ties
    floor = np.maximum(np.floor(rare.astype(np.float64) * (1 << bits)), rare > 0).astype(np.int64)[0]
    want = floor.copy()
    want[3] += (1 << bits) - floor.sum()
    assert want[3] >= 1 and np.array_equal(freq[3], want)  # at 8 bits the 50 forced ones overshoot: taken from entry 3 again
    c = R.cumulative(freq)
    assert np.all(c[:, 0] == 0) and np.array_equal(c[:, 1:], np.cumsum(freq, axis=1)[:, :-1])


def test_frequency_normaliser_refuses_bad_tables():
    for bad in (np.zeros((1, 256), np.float32), np.full((1, 256), np.nan, np.float32), -np.ones((1, 256), np.float32),
                np.ones((1, 255), np.float32)):
        with pytest.raises(ValueError):
            R.normalize_frequencies(bad)
    with pytest.raises(ValueError):
        R.normalize_frequencies(np.ones((1, 256), np.float32), bits=15)


@pytest.mark.parametrize("n", [1, S - 1, S, S + 1])
def test_numpy_coder_round_trip(n):
    """Channel 0: a single symbol (frequency = M, no byte is ever emitted); 1: two symbols, one of them once; 2: all 256 present
    (when n allows); 3: uniform noise."""
    rng = np.random.default_rng(n)
    sym = np.zeros((n, 4), np.uint8)
    sym[:, 0] = 77
    sym[:, 1] = 200
    sym[n // 2, 1] = 9
    sym[:, 2] = rng.permutation(np.arange(n) % 256)
    sym[:, 3] = rng.integers(0, 256, n)
    prob = probabilities(sym)
    blob = R.encode(sym, prob, stream_len=S)
    bits, channels, stream_len, count, offsets, payload = R.parse_container(blob)
    n_streams = -(-n // S)
    assert (bits, channels, stream_len, count) == (14, 4, S, n) and offsets.size == 4 * n_streams + 1
    assert np.all(np.diff(offsets)[:n_streams] == 4)  # the single-symbol channel: the state alone, and it never left L
    assert np.all(payload[:4 * n_streams].view("<u4") == R.STATE_LOW)
    assert np.array_equal(R.decode(blob, prob), sym)
    assert np.array_equal(R.decode(blob.tobytes(), prob), sym)
    for other_len in (64, 100):
        assert np.array_equal(R.decode(R.encode(sym, prob, stream_len=other_len, bits=12), prob), sym)
    with pytest.raises(ValueError):  # a symbol the table gives no probability
        R.encode(np.full((n, 4), 5, np.uint8), prob, stream_len=S)


def test_streams_are_independent_and_forward():
    """Stream k holds symbols [k S, (k + 1) S) of its channel: decoding a container cut down to one stream gives that slice."""
    sym = draw("gaussian", 5 * 64 + 3, 2)
    prob = probabilities(sym)
    bits, c, s, n, offsets, payload = R.parse_container(R.encode(sym, prob, stream_len=64))
    k = 4  # the 5th stream of channel 1: [256, 320)
    sid = 1 * 6 + k
    one = R.build_container(bits, 1, 64, 64, np.array([0, offsets[sid + 1] - offsets[sid]]), payload[offsets[sid]:offsets[sid + 1]])
    assert np.array_equal(R.decode(one, prob[1:2])[:, 0], sym[256:320, 1])


def test_container_validation():
    sym = draw("peaked", 3 * 64 + 1, 2)
    prob = probabilities(sym)
    blob = R.encode(sym, prob, stream_len=64)
    head = struct.calcsize("<8sIIIIQ")
    n_off = 2 * 4 + 1

    def with_offsets(fn):
        b = blob.copy()
        off = b[head:head + 4 * n_off].view("<u4").copy()
        fn(off)
        b[head:head + 4 * n_off] = off.view(np.uint8)
        return b

    wrong_magic = blob.copy()
    wrong_magic[:8] = np.frombuffer(np.arange(2, dtype="<u4").tobytes(), np.uint8)
    foreign = np.random.default_rng(0).integers(0, 2**32, 500, dtype=np.uint32)  # what a `constriction` stream looks like: words
    for bad in (wrong_magic, foreign, foreign.tobytes(), b"", blob[:4]):
        with pytest.raises(ValueError, match="not interchangeable"):
            R.decode(bad, prob)
    decreasing = with_offsets(lambda off: off.__setitem__(3, off[2] - 1))
    too_short = with_offsets(lambda off: off.__setitem__(3, off[2] + 3))
    past_end = with_offsets(lambda off: off.__setitem__(n_off - 1, off[n_off - 1] + 1))
    not_from_zero = with_offsets(lambda off: off.__setitem__(0, 1))
    truncated = blob[:-5]
    no_table = blob[:head + 7]
    version = blob.copy()
    version[8] = 2
    resolution = blob.copy()
    resolution[12] = 20
    for bad in (decreasing, too_short, past_end, not_from_zero, truncated, no_table, blob[:head - 1], version, resolution):
        with pytest.raises(ValueError):
            R.parse_container(bad)
        with pytest.raises(ValueError):
            R.decode(bad, prob)
    with pytest.raises(ValueError):  # three rows of probabilities for two channels
        R.decode(blob, np.concatenate([prob, prob[:1]]))
    assert np.array_equal(R.decode(blob, prob), sym)


def test_damaged_payload_decodes_to_something():
    """Flipped payload bytes give wrong symbols, not an error: reads stay inside each stream and are 0 beyond it."""
    sym = draw("uniform", 300, 1)
    prob = probabilities(sym)
    blob = R.encode(sym, prob, stream_len=64)
    bad = blob.copy()
    bad[-40:] = 255 - bad[-40:]
    out = R.decode(bad, prob)
    assert out.shape == sym.shape and out.dtype == np.uint8 and np.array_equal(out[:192], sym[:192])


def test_container_bytes_are_pinned():
    """The whole file, byte for byte, for N around one and several streams of S = 5 at P = 8, 12 and 14: arrays recorded by
    tests/golden/make_golden_ans_containers.py from the coder as it stood before the stream layer was shared."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ans_containers.npz"))
    for n in (1, 4, 5, 6, 17):
        sym, prob = g[f"f.{n}.sym"], g[f"f.{n}.prob"]
        assert sym.shape == (n, 3) and sym.dtype == np.uint8 and prob.dtype == np.float32
        for bits in (8, 12, 14):
            blob = g[f"f.{n}.{bits}.blob"]
            got = R.encode(sym, prob, stream_len=5, bits=bits)
            assert got.dtype == np.uint8 and np.array_equal(got, blob), (n, bits)
            assert np.array_equal(R.decode(blob, prob), sym), (n, bits)


@pytest.mark.parametrize("kind", DISTRIBUTIONS)
def test_size_bound_numpy_coder(kind):
    """file bytes <= 1.01 x empirical entropy + 8 bytes per stream + 64, on 16384 symbols at S = 1024.  Measured for this coder
    at P = 14: payload net of the 4-byte states / entropy between 0.996 and 1.000 on the three distributions."""
    sym = draw(kind, 16384, 1)
    blob = R.encode(sym, probabilities(sym), stream_len=S)
    print(f"{kind}: {blob.size} bytes, entropy {entropy_bytes(sym):.1f} bytes, bound {size_bound(sym, S):.1f}")
    assert blob.size <= size_bound(sym, S)
