"""The base64url frame codec at its lane, wave, block and padding seams, byte for byte.

k_b64url_encode_frame / k_b64url_encode_frames (publish_partial,
publish_partials) and k_b64url_decode (ingest_pubsub) over the cases of
tests/codec_cases.py; tests/test_codec_cases.py shows on the CPU what those
cases reach and that they tell a wrong decomposition from the right one.
Expected texts, bytes and statuses come from the oracle alone
(frame_encode's header, java_b64url_encode, java_b64url_decode,
pubsub_decode, frame_decode and the status rule codec_cases.ingest_expected);
frames are built from the planted 64-bit patterns, never from a value read
back.  (Division of labour: large texts and the grid-stride loop in
test_gpu_multi.py, random mutations of texts in test_gpu_parity.py, the seams
here.)

Encoder.  One handle of three partitions per payload length: partition 0
stays logically +0.0, 1 and 2 hold arbitrary bit patterns (NaN payloads,
infinities, both zeros, subnormals) in W.  W has no zero flag, so its
partition 0 is read from memory like any other; the null-source path of the
kernel is reached through AGG of the same handle, which nothing has written.
Device texts lie between bands of 0xAB at a 16-B aligned address and one byte
past it (the scratch-and-copy path) with the capacity set to the text length;
the whole buffer is fetched and compared, bands and the gaps of a batch
included.

Decoder.  Through the C-ABI the decoder's output can be observed only where
the fold consumes it: the first L_p payload doubles of a frame, and the
per-message status.  The decoded origin bytes cannot be checked, and a text
with an origin shows only its status and the payload before its tail.  Every
message goes to a partition of its own whose AGG is logically zero, so
read(p) is +0.0 + x for every payload double, bit for bit (finite patterns:
-0.0 becomes +0.0, nothing else changes), and one wrong byte of one message
shows.
"""
import numpy as np
import pytest

import codec_cases as C

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FILL, GUARD = C.FILL, C.GUARD


@pytest.fixture(scope="module")
def ipls():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu run without a visible GPU")
    import ipls as m
    return m


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as o   # checker only
    return o


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want, what):
    got, want = u64(got), np.ascontiguousarray(want, dtype=np.uint64)
    assert got.shape == want.shape, f"{what}: {got.shape} != {want.shape}"
    bad = np.flatnonzero(got != want)
    assert not bad.size, f"{what}: {bad.size} of {got.size} differ; first at {bad[0]}: {got[bad[0]]:#018x} != {want[bad[0]]:#018x}"


def same_text(got, want, what):
    got, want = bytes(got), bytes(want)
    if got != want:
        n = min(len(got), len(want))
        i = next((i for i in range(n) if got[i] != want[i]), n)
        raise AssertionError(f"{what}: lengths {len(got)} / {len(want)}, first difference at char {i} "
                             f"(group {i // C.GROUP_CHARS}): {got[i - 4:i + 8]!r} != {want[i - 4:i + 8]!r}")


class DeviceText:
    """A device byte buffer for texts of up to `cap` bytes between two bands of GUARD bytes, all 0xAB before a call."""

    def __init__(self, cap):
        self.t = torch.empty(GUARD + cap + 16 + GUARD, dtype=torch.uint8, device="cuda")
        assert int(self.t.data_ptr()) % 16 == 0 and GUARD % 16 == 0

    def at(self, shift):
        self.shift = shift
        self.t.fill_(FILL)
        torch.cuda.synchronize()   # the fill ran on torch's stream; the handle's does not order after it
        return int(self.t.data_ptr()) + GUARD + shift

    def check(self, agg, placed, what):
        """The whole buffer is 0xAB but for the texts [(offset, text)]."""
        agg.sync()
        got = self.t.cpu().numpy()
        want = np.full(got.size, FILL, dtype=np.uint8)
        lo = GUARD + self.shift
        for off, text in placed:
            want[lo + off:lo + off + len(text)] = np.frombuffer(text, dtype=np.uint8)
        bad = np.flatnonzero(got != want)
        if bad.size:
            i = int(bad[0]) - lo
            where = "before the first text" if i < 0 else f"at offset {i}"
            raise AssertionError(f"{what}: {bad.size} bytes differ, first {where}: {got[bad[0]]:#04x} != {want[bad[0]]:#04x}")


def check_batch(ipls, agg, dev, pin, parts, a, bs, pid, origin, target, texts, what):
    """publish_partials into host memory, pinned memory and guarded device memory: the texts, their 64-B layout, the gaps."""
    kw = dict(pid=pid, origin=origin, target=target)
    got = agg.publish_partials(parts, a, bs, **kw)
    assert len(got) == len(texts)
    for p, g, t in zip(parts, got, texts):
        same_text(g, t, f"{what}: batch host text of partition {p}")
    lens = [len(t) for t in texts]
    offs, end = C.batch_layout(lens)
    v = pin.view()
    v[:] = FILL
    assert agg.publish_partials(parts, a, bs, out=pin, **kw) == (lens, offs), f"{what}: pinned layout"
    want = np.full(v.size, FILL, dtype=np.uint8)
    for o, t in zip(offs, texts):
        want[o:o + len(t)] = np.frombuffer(t, dtype=np.uint8)
    bad = np.flatnonzero(v != want)
    assert not bad.size, f"{what}: pinned batch differs at offset {bad[0]}: {v[bad[0]]:#04x} != {want[bad[0]]:#04x}"
    for shift in (0, 1):
        addr = dev.at(shift)
        assert agg.publish_partials(parts, a, bs, out=addr, out_cap=end, **kw) == (lens, offs), f"{what}: device layout"
        dev.check(agg, list(zip(offs, texts)), f"{what}: device batch at 16-B + {shift}")


# ---------------------------------------------------------------------------
# encoder
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.encoder_ns())
def test_encoder_seams(ipls, O, n):
    W, AGG = ipls.TGT_WEIGHTS, ipls.TGT_AGG
    origins = C.origins_of(n)
    agg = ipls.Aggregator(n_partitions=3, bucket_len=n)
    vals = [np.zeros(n, dtype=np.uint64), C.enc_values(n, 1), C.enc_values(n, 2)]
    for p in (1, 2):
        agg.cache_partition(p, vals[p].view(np.float64))
    for p in range(3):
        same_bits(agg.read(p, W), vals[p], f"n={n}: planted W[{p}]")
    cap = C.batch_layout([C.text_len(C.frame_len(n, max(origins)))] * 3)[1]
    dev, pin = DeviceText(cap), ipls.PinnedBuffer(cap + 64)
    for o in origins:
        a, bs, pid = C.enc_header(n, o)
        origin = C.enc_origin(n, o)
        want = [O.java_b64url_encode(C.frame_bytes(O, vals[p], a, bs[p], pid, origin)) for p in range(3)]
        for p, tgt in ((0, W), (0, AGG), (1, W), (2, W)):
            what = f"n={n} o={o} p={p} target={tgt}"
            kw = dict(pid=pid, origin=origin, target=tgt)
            same_text(agg.publish_partial(p, a, bs[p], **kw), want[p], f"{what}: host text")
            for shift in (0, 1):
                addr = dev.at(shift)
                assert agg.publish_partial(p, a, bs[p], out=addr, out_cap=len(want[p]), **kw) == len(want[p]), what
                dev.check(agg, [(0, want[p])], f"{what}: device text at 16-B + {shift}")
        order = [2, 0, 1]
        check_batch(ipls, agg, dev, pin, order, a, [bs[p] for p in order], pid, origin, W, [want[p] for p in order],
                    f"n={n} o={o} W")
        zero = [O.java_b64url_encode(C.frame_bytes(O, vals[0], a, bs[p], pid, origin)) for p in order]
        got = agg.publish_partials(order, a, [bs[p] for p in order], pid=pid, origin=origin, target=AGG)
        for p, g, t in zip(order, got, zero):
            same_text(g, t, f"n={n} o={o}: batch text of the logically zero AGG[{p}]")
    pin.close()
    agg.close()


def test_encoder_model_geometry_batch(ipls, O):
    """Aggregator(M, P) over two shards of one GPU: partitions of 193 doubles
    and a last one of 3, so one launch holds jobs of 3 and of more than 64
    groups, on both shards."""
    W = ipls.TGT_WEIGHTS
    M, P = C.ENC_MODEL
    agg = ipls.Aggregator(M, P, devices=[0, 0])
    assert agg.lengths == C.model_lengths(M, P)
    parts = list(C.ENC_MODEL_BATCH)
    vals = {p: C.enc_values(agg.lengths[p], 3 + p) for p in parts}
    for p in parts:
        agg.cache_partition(p, vals[p].view(np.float64))
        same_bits(agg.read(p, W), vals[p], f"planted W[{p}]")
    cap = C.batch_layout([C.text_len(C.frame_len(193, 46))] * len(parts))[1]
    dev, pin = DeviceText(cap), ipls.PinnedBuffer(cap + 64)
    for o in (0, 13, 46):
        a, bs5, pid = C.enc_header(193, o)[0], [int(x) for x in range(-2, 3)], C.enc_header(193, o)[2]
        origin = C.enc_origin(193, o)
        want = [O.java_b64url_encode(C.frame_bytes(O, vals[p], a, b, pid, origin)) for p, b in zip(parts, bs5)]
        for p, b, t in zip(parts, bs5, want):
            same_text(agg.publish_partial(p, a, b, pid=pid, origin=origin, target=W), t, f"model o={o} p={p}: host text")
        check_batch(ipls, agg, dev, pin, parts, a, bs5, pid, origin, W, want, f"model o={o}")
    pin.close()
    agg.close()


# ---------------------------------------------------------------------------
# decoder
# ---------------------------------------------------------------------------
def ingest_exact(agg, O, msgs, layers, p0, what):
    """Message i of [(text, planted bits)] into partition p0 + i: status 0 each, read-back +0.0 + x by bits."""
    parts = list(range(p0, p0 + len(msgs)))
    for (text, bits), p in zip(msgs, parts):
        st, dec = C.ingest_expected(O, text, layers, agg.n_partitions, agg.lengths, p)
        assert st == 0 and (u64(dec[1])[:bits.size] == bits).all(), f"{what}: the oracle does not give back message {p - p0}"
    k, st = agg.ingest_pubsub([m[0] for m in msgs], layers=layers, partitions=parts)
    assert st == [0] * len(msgs), f"{what}: statuses {[(i, s) for i, s in enumerate(st) if s]}"
    assert k == len(msgs), what
    for (text, bits), p in zip(msgs, parts):
        same_bits(agg.read(p), C.folded_bits(bits), f"{what}: message {p - p0} ({len(text)} chars)")


@pytest.mark.parametrize("L", C.DEC_LS)
def test_decoder_sweep(ipls, O, L):
    one = [(t, b) for t, b, o, dc in C.sweep_messages(O, L, 1)]
    two = [(t, b) for t, b, o, dc in C.sweep_messages(O, L, 2)]
    agg = ipls.Aggregator(n_partitions=len(one) + len(two), bucket_len=L)
    ingest_exact(agg, O, one, 1, 0, f"L={L} one layer")
    ingest_exact(agg, O, two, 2, len(one), f"L={L} two layers")
    agg.close()


@pytest.mark.parametrize("L", C.ALPHA_LS)
def test_decoder_alphabet(ipls, O, L):
    msgs = C.alphabet_messages(O, L)
    agg = ipls.Aggregator(n_partitions=len(msgs), bucket_len=L)
    ingest_exact(agg, O, msgs, 1, 0, f"alphabet L={L}")
    agg.close()


def test_decoder_discarded_tail_bits(ipls, O):
    """Java ignores the low bits of the last char of a two- or three-char tail: the same bytes, status 0."""
    groups = {}
    for text, bits, layers in C.discarded_bits_messages(O):
        groups.setdefault((bits.size, layers), []).append((text, bits))
    assert {k for k in groups} >= {(4, 1), (4, 2), (6, 1), (6, 2)}
    for (L, layers), msgs in groups.items():
        agg = ipls.Aggregator(n_partitions=len(msgs), bucket_len=L)
        ingest_exact(agg, O, msgs, layers, 0, f"discarded bits L={L} layers={layers}")
        agg.close()


@pytest.mark.parametrize("layer", ["outer", "inner"])
def test_decoder_every_invalid_byte(ipls, O, layer):
    """Each of the 192 byte values outside the alphabet at each position
    class of the layer, one per message, a valid message after every third.
    The oracle's rule gives the status (-6, but for a '=' where Java stops and
    accepts); what folds comes back exact, what does not leaves its partition
    +0.0, and the fold count is the number of zeros."""
    L, P = C.INVALID_L, 256
    agg = ipls.Aggregator(n_partitions=P, bucket_len=L)
    batches = C.invalid_batches(O)
    for cname in C.invalid_class_names():
        msgs = batches[(layer, cname)]
        what = f"{layer} {cname}"
        agg.reset()
        exp = [C.ingest_expected(O, m[0], 2, P, agg.lengths, i) for i, m in enumerate(msgs)]
        assert all(e[0] == 0 for e, m in zip(exp, msgs) if m[2] is None) and [e[0] for e in exp].count(-6) >= 188
        k, st = agg.ingest_pubsub([m[0] for m in msgs], layers=2, partitions=list(range(len(msgs))))
        bad = [(i, msgs[i][2], e[0], st[i]) for i, e in enumerate(exp) if st[i] != e[0]]
        assert not bad, f"{what}: (index, (byte, origin, data chars, position), expected, got): {bad[:8]}"
        assert k == [e[0] for e in exp].count(0), what
        for i, (e, m) in enumerate(zip(exp, msgs)):
            if e[0] == 0:
                if m[2] is None:
                    assert (u64(e[1][1]) == m[1]).all()
                same_bits(agg.read(i), C.folded_bits(u64(e[1][1])[:L]), f"{what}: message {i}")
            else:
                assert not u64(agg.read(i)).any(), f"{what}: message {i} was refused and yet its partition changed"
    agg.close()
