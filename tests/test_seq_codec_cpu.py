"""CPU: the numpy module that defines the plane-sequence format of SeqHevcCompression
(gscodec_studio_amd/compression/plane_seq_codec_reference.py) -- the closed loop without drift, what it shares with the per-plane
codec, the coefficient bound for signed input, the lossless means wrapper, every refusal of the parser, and the rate condition on
the drifting garden planes."""
import struct

import numpy as np
import pytest

from plane_codec_cases import psnr
from seq_codec_cases import CASE_IDS, QPS, case_frames, case_of, garden_sequences, reference_blob, reference_levels
from gscodec_studio_amd.compression import plane_codec_reference as P
from gscodec_studio_amd.compression import plane_seq_codec_reference as R


@pytest.mark.parametrize("name", CASE_IDS)
def test_decoder_state_equals_encoder_state(name):
    """decode(encode(x)) = reconstruct(x): no drift on any frame; the levels' escapes survive the file."""
    gop = case_of(name)[6]
    x = case_frames(name)
    for qp in QPS:
        levels, frames = reference_levels(name, qp)
        assert np.array_equal(R.forward_levels(x, qp, gop), levels) and np.array_equal(R.reconstruct(x, qp, gop), frames)
        assert np.array_equal(R.inverse_levels(levels, qp, gop, x.shape[1], x.shape[2]), frames), (name, qp)
        blob = reference_blob(name, qp, 4096)
        assert np.array_equal(R.decode(blob), frames), (name, qp)
    assert np.array_equal(R.decode(reference_blob(name, 22, 64).tobytes()), reference_levels(name, 22)[1])  # bytes or an array


@pytest.mark.parametrize("name", [n for n in CASE_IDS if case_of(n)[6] == 1 or case_of(n)[5] == 1])
def test_intra_frames_are_the_plane_codec(name):
    """gop = 1, and T = 1: every decoded frame is the plane codec's, the I group's symbols are the per-frame plane symbols."""
    x, gop = case_frames(name), case_of(name)[6]
    for qp in QPS:
        levels, frames = reference_levels(name, qp)
        for t in range(x.shape[0]):
            assert np.array_equal(frames[t], P.reconstruct(x[t], qp)) and np.array_equal(levels[t], P.forward_levels(x[t], qp))
        (sym, esc), group_p = R.levels_to_symbols(levels, gop)
        per_frame = [P.levels_to_symbols(P.forward_levels(x[t], qp)) for t in range(x.shape[0])]
        assert group_p is None
        assert np.array_equal(sym, np.concatenate([s for s, _ in per_frame])) and np.array_equal(esc, np.concatenate([e for _, e in per_frame]))


def test_single_frame_file_is_the_plane_file_behind_the_header():
    x = case_frames([n for n in CASE_IDS if case_of(n)[5] == 1 and case_of(n)[2:4] == (9, 17)][0])
    blob, plane_blob = R.encode(x, 22, 5), P.encode(x[0], 22)
    assert np.array_equal(blob[R._HEADER.size:], plane_blob[P._HEADER.size:])


def test_p_frames_keep_their_dc_levels_and_escape():
    x = case_frames([n for n in CASE_IDS if n.startswith("flip-5x24x24")][0])
    levels = R.forward_levels(x, 0, 6)
    (sym_i, esc_i), (sym_p, esc_p) = R.levels_to_symbols(levels, 6)
    assert sym_i.size == 64 * levels.shape[1] * 9 and sym_p.size == 4 * sym_i.size
    u = 2 * np.abs(levels[1:].astype(np.int64)) - (levels[1:] < 0)  # no DC differences in the P group
    assert np.array_equal(sym_p, np.minimum(u, 255).reshape(-1)) and esc_p.size == int((u >= 255).sum()) > 0
    back = R.symbols_to_levels((sym_i, esc_i), (sym_p, esc_p), 5, 6, levels.shape[1])
    assert np.array_equal(back, levels)


def test_coefficient_bound_for_signed_input():
    """|coefficient| <= 32640 for residuals in -255..255: the flip cases' residuals, every sign pattern of two rows of M, +-255."""
    worst = 0
    for name in CASE_IDS:
        content, frames = case_of(name)[1], case_of(name)[5]
        if content in ("flip", "checker-flip") and frames > 1:
            x = case_frames(name)
            res = P._blocks(x[1]) - P._blocks(x[0])
            assert np.abs(res).max() == 255
            worst = max(worst, int(np.abs(P.transform_blocks(res)).max()), int(np.abs(P.transform_blocks(-res)).max()))
    sign = np.where(P.M >= 0, 1, -1)
    patterns = 255 * (sign[:, None, :, None] * sign[None, :, None, :]).reshape(1, 64, 8, 8)  # maximises coefficient (v, u)
    for res in (patterns, -patterns, np.full((1, 1, 8, 8), 255), np.full((1, 1, 8, 8), -255)):
        worst = max(worst, int(np.abs(P.transform_blocks(res)).max()))
    assert worst == 32640
    assert int(np.abs(P.M).sum(axis=1).max()) <= 512
    # and the quantiser's product stays in int32 at every qp
    assert 32640 * max(P.QS) + (171 << (18 + 51 // 6 - 9)) < 1 << 31


def test_means_wrapper_is_lossless():
    rng = np.random.default_rng(11)
    for shape, gop in (((1, 5, 7, 3), 1), ((4, 6, 6, 3), 4), ((5, 3, 9, 3), 2), ((3, 4, 4, 1), 250), ((3, 4, 4, 3), 1)):
        g = rng.integers(0, 65536, shape).astype(np.uint16)
        if shape[0] > 1:  # a walk of small steps with wrap-around in both directions: 0 <-> 65535 between frames
            g[1:] = g[0] + rng.integers(-3, 4, (shape[0] - 1,) + shape[1:]).cumsum(axis=0).astype(np.uint16)
            g[0, 0, 0, 0], g[1, 0, 0, 0] = 0, 65535
            g[0, 0, 1, 0], g[1, 0, 1, 0] = 65535, 0
            g[0, 1, 0, 0], g[1, 1, 0, 0] = 0, 32768  # the int16 minimum
        blob = R.encode_means(g, gop, stream_len=64)
        assert np.array_equal(R.decode_means(blob), g), (shape, gop)
        head = R.parse_means_container(blob)[0]
        assert (head.frames, head.height, head.width, head.channels, head.gop) == shape + (gop,)
        assert (head.bytes_p == 0) == (gop == 1 or shape[0] == 1)
    sym_i, sym_p = R.means_symbols(g, 2)  # g: three frames, gop 1 above; with gop 2 frame 1 is a difference
    assert sym_i.shape == (2 * 16, 6) and sym_p.shape == (16, 6)
    small = rng.integers(0, 65536, (6, 16, 16, 3)).astype(np.uint16)
    small[1:] = small[0] + rng.integers(-2, 3, (5, 16, 16, 3)).cumsum(axis=0).astype(np.uint16)
    assert R.encode_means(small, 6).size < R.encode_means(small, 1).size  # differences of a slow walk cost less than raw values
    for bad, gop in ((small.astype(np.int32), 2), (small[0], 2), (small, 0), (small[:0], 1)):
        with pytest.raises(ValueError):
            R.encode_means(bad, gop)
    blob = R.encode_means(small, 3)
    for damaged, match in ((blob[:-1], "name"), (np.concatenate([blob, blob[:2]]), "behind the last group"), (b"x" * 64, "magic"),
                           (blob[:20], "truncated")):
        with pytest.raises(ValueError, match=match):
            R.decode_means(damaged, what="name")


def _with_header(blob, **changes):
    fields = list(struct.unpack("<11I", blob[8:R._HEADER.size].tobytes()))
    names = ("version",) + R.Header._fields
    for k, v in changes.items():
        fields[names.index(k)] = v
    return np.concatenate([np.frombuffer(R.MAGIC + struct.pack("<11I", *fields), np.uint8), blob[R._HEADER.size:]])


def test_parser_refuses_what_a_decoder_must_not_start_on():
    x = case_frames([n for n in CASE_IDS if n.startswith("noise-5x9x17")][0])
    blob = R.encode(x, 0, 2, stream_len=64)  # escapes in both groups
    head, group_i, group_p = R.parse_container(blob)
    assert head.n_escapes_i > 0 and head.n_escapes_p > 0 and group_p is not None
    assert (head.frames, head.gop, head.height, head.width, head.channels, head.qp, head.stream_len) == (5, 2, 9, 17, x.shape[3], 0, 64)

    def refused(damaged, match):
        with pytest.raises(ValueError, match=match) as e:
            R.parse_container(damaged, what="seq.bin")
        assert "seq.bin" in str(e.value)

    refused(P.encode(x[0], 0), "magic")  # the per-plane container is another format
    refused(blob[:6], "magic")
    refused(blob[:30], "truncated plane-sequence header")
    refused(_with_header(blob, version=2), "version 2")
    for field, value in (("bits", 7), ("bits", 15), ("stream_len", 0), ("stream_len", (1 << 24) + 1), ("qp", 52), ("channels", 0), ("channels", 5)):
        refused(_with_header(blob, **{field: value}), "bad plane-sequence header")
    refused(_with_header(blob, frames=0), "T = 0")
    refused(_with_header(blob, gop=0), "gop = 0")
    refused(_with_header(blob, height=0), "H = 0")
    refused(_with_header(blob, height=1 << 15, width=1 << 14, frames=4, gop=1), "bad plane-sequence header")  # 2^31 in the I group
    refused(_with_header(blob, height=1 << 15, width=1 << 14, frames=8, gop=2), "bad plane-sequence header")  # 2^31 in either
    # tables
    pos = R._HEADER.size
    refused(blob[:pos + 1], "truncated or empty frequency table of context 0")
    bad = blob.copy(); bad[pos:pos + 2] = 0
    refused(bad, "truncated or empty frequency table of context 0")
    bad = blob.copy(); bad[pos + 3] ^= 1  # a frequency of the first table
    refused(bad, "does not sum")
    count = int(blob[pos:pos + 2].view("<u2")[0])
    if count > 1:
        bad = blob.copy(); bad[pos + 2], bad[pos + 5] = blob[pos + 5], blob[pos + 2]
        refused(bad, "out of order")
    # offsets of the I group
    tables_end = len(R.MAGIC) + 44 + len(P._pack_tables(group_i.freq))
    assert np.array_equal(blob[tables_end:tables_end + 4 * group_i.offsets.size].view("<u4"), group_i.offsets)
    refused(blob[:tables_end + 5], "truncated ANS offset table")
    bad = blob.copy(); bad[tables_end:tables_end + 4].view("<u4")[0] = 1
    refused(bad, "must start at 0")
    bad = blob.copy(); bad[tables_end + 4:tables_end + 8].view("<u4")[0] = 3
    refused(bad, "at least its 4 state bytes")
    bad = blob.copy(); bad[tables_end + 4 * (group_i.offsets.size - 1):tables_end + 4 * group_i.offsets.size].view("<u4")[0] = blob.size
    refused(bad, "past the end of the file")
    # groups against T and gop; the end of the file
    end_i = tables_end + 4 * group_i.offsets.size + int(group_i.offsets[-1]) + 2 * head.n_escapes_i
    refused(blob[:end_i], "imply a P group")
    refused(blob[:end_i - 1], "escapes of 2 bytes")
    refused(blob[:-1], "escapes of 2 bytes")
    refused(np.concatenate([blob, blob[:2]]), "behind the last group")
    refused(_with_header(blob, n_escapes_p=head.n_escapes_p - 1), "behind the last group")
    refused(_with_header(blob, n_escapes_p=head.n_escapes_p + 1), "escapes of 2 bytes")
    intra = R.encode(x, 0, 1, stream_len=64)
    assert R.parse_container(intra)[2] is None
    refused(np.concatenate([intra, blob[end_i:]]), "leave no P frame")  # a P group that T and gop exclude
    refused(_with_header(intra, n_escapes_p=1), "leave none")
    # a file of gop 2 read as gop 3: other group sizes, other offset tables -- refused by one check or another, never decoded
    with pytest.raises(ValueError):
        R.parse_container(_with_header(blob, gop=3))


@pytest.mark.parametrize("name", [n for n in CASE_IDS if case_of(n)[2:4] == (100, 100)])
def test_file_ends_where_the_offsets_say(name):
    frames, gop = case_of(name)[5:7]
    for s_len in (64, 4096):
        blob = reference_blob(name, 22, s_len)
        head, group_i, group_p = R.parse_container(blob)
        n_i = -(-frames // gop)
        per_frame = 64 * head.channels * 169
        size = R._HEADER.size
        for group, n_frames, n_esc in ((group_i, n_i, head.n_escapes_i), (group_p, frames - n_i, head.n_escapes_p)):
            if group is None:
                assert n_frames == 0
                continue
            assert group.offsets.size == -(-per_frame * n_frames // s_len) + 1 and group.escapes.size == n_esc
            assert group.payload.size == int(group.offsets[-1])
            size += len(P._pack_tables(group.freq)) + 4 * group.offsets.size + group.payload.size + 2 * n_esc
        assert size == blob.size


def test_encode_refuses_bad_arguments():
    x = case_frames(CASE_IDS[0])
    for frames, qp, gop in ((x.astype(np.int16), 4, 2), (x[0, :, :, 0], 4, 2), (x[:0], 4, 2), (x, 52, 2), (x, -1, 2), (x, 4, 0), (x, 4, True),
                            (x, 4, 1.5), (np.zeros((1, 8, 8, 5), np.uint8), 4, 1)):
        with pytest.raises(ValueError):
            R.encode(frames, qp, gop)
    with pytest.raises(ValueError, match="stream_len"):
        R.encode(x, 4, 1, stream_len=0)
    assert R.decode(R.encode(x[..., 0], 4, 1)).shape == x.shape[:3] + (1,)  # [T, H, W] is one channel


def test_rate_condition_on_the_drifting_garden_planes():
    """T = 6, drift sigma = 1.5: predicting from the frame before (gop 6) against all-intra (gop 1).  The caps are the issue's:
    at most 0.6 of the all-intra bytes at qp 22 and 34, strictly fewer at qp 4, and a worst frame at most 0.5 dB below all-intra's."""
    for name, x in garden_sequences().items():
        for qp, cap in ((4, None), (22, 0.6), (34, 0.6)):
            inter, intra = R.encode(x, qp, 6), R.encode(x, qp, 1)
            ratio = inter.size / intra.size
            worst = [min(psnr(x[t], rec[t]) for t in range(6)) for rec in (R.decode(inter), R.decode(intra))]
            print(f"{name} qp {qp}: gop 6 {inter.size} B, gop 1 {intra.size} B, ratio {ratio:.3f}; worst frame PSNR {worst[0]:.2f} dB against {worst[1]:.2f} dB")
            assert inter.size < intra.size and (cap is None or ratio <= cap), (name, qp, ratio)
            assert worst[0] >= worst[1] - 0.5, (name, qp, worst)
