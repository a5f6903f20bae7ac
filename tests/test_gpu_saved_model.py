"""Saved-model files on the GPU: ipls_agg_save_model (+ _chunked),
ipls_agg_save_partition, ipls_agg_save_model_list, ipls_agg_load_saved, the
IPLS_HOST_DLIST model load and the IPLS_HOST_DARR source kind against the
writer restated in tests/saved_model_writer.py (byte for byte, NaN positions
included) and the oracle's blend.

Shapes: synthetic handles whose partition length L is 1, 2, 3, 7 and the pack /
apply kernels' tile (kSerTileWords 16-B words = 2,048 doubles) - 1, + 0, + 1
and 2 tiles + 3, with P = 3 and P = 5 (payloads at 5 and 1 mod 8, every
residue mod 16 over the L's), and the reference geometry M = 30,011 with 3
partitions; the last also on a two-shard handle (both shards on GPU 0).
References: IPLS.java:1904-1911 (save_model), 728-731 + Updater.java:65-69
(DownloadMapParameters, the leaving-peer blend), 136-140 (the double[] file),
547-558 / 2255-2273 (the ArrayList<Double>), 567 + 1880-1901 (its load).
"""
import ctypes
import subprocess

import numpy as np
import pytest

import saved_model_writer as W
from conftest import ROOT, assert_bits_equal
from oracle import javaser as J

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TILE = 2048          # doubles per block-tile of k_ser_pack / k_ser_apply (kBlock * kSerV 16-B words)
RANGE, FORMAT = -2, -6


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


def _open(ipls, shape, devices=None):
    kind, a, b = shape
    if kind == "synthetic":
        return ipls.Aggregator(n_partitions=b, bucket_len=a, devices=devices)
    return ipls.Aggregator(a, b, devices=devices)


def _ubits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _exact(a, b, what):
    """Bit equality with no NaN allowance: a double[] payload keeps raw bits."""
    assert np.array_equal(_ubits(a), _ubits(b)), what


def _weights(agg, seed):
    return [W.edge_values(L, seed + 7 * p) for p, L in enumerate(agg.lengths)]


def _place(agg, w):
    for p, x in enumerate(w):
        agg.cache_partition(p, x)


def _all(agg, ipls):
    return [agg.read(p, ipls.TGT_WEIGHTS) for p in range(agg.n_partitions)]


def _collect(agg, parts, chunk):
    got, offs = bytearray(), []

    def sink(ptr, off, cnt):
        assert off == len(got) and 0 < cnt <= chunk
        offs.append(off)
        got.extend(ctypes.string_at(ptr, cnt))
        agg.partition_len(0)                    # the sink may call back into the handle
        return True
    assert agg.save_model(parts, sink=sink, chunk_bytes=chunk) is None
    return bytes(got), offs


SYNTH = [("synthetic", L, P) for P in (3, 5) for L in (1, 2, 3, 7, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)]
MODEL = ("model", 30011, 3)
CASES = [(s, None) for s in SYNTH] + [(MODEL, None), (MODEL, [0, 0]), (("synthetic", 7, 5), [0, 0]),
                                      (("synthetic", TILE + 1, 3), [0, 0])]
IDS = [f"{s[0]}-{s[1]}x{s[2]}" + ("-2shards" if d else "") for s, d in CASES]


@pytest.mark.parametrize("shape,devices", CASES, ids=IDS)
def test_save_bytes_equal_the_restated_writer(ipls, shape, devices):
    with _open(ipls, shape, devices) as agg:
        P = agg.n_partitions
        # a fresh accumulator is logically +0.0: its payload is +0.0 bytes
        zeros = {p: np.zeros(agg.lengths[p]) for p in range(P)}
        assert agg.save_model(target=ipls.TGT_AGG) == W.write_map(zeros, range(P))
        assert agg.save_partition(P - 1, target=ipls.TGT_REP) == W.write_darr(zeros[P - 1])
        w = _weights(agg, 11)
        _place(agg, w)
        wd = dict(enumerate(w))
        whole = W.write_map(wd, range(P))
        assert agg.save_model() == whole
        back = [P - 1, 0, P - 1]                                    # Auth_List order, one listed twice
        assert agg.save_model(back) == W.write_map(wd, back)
        assert agg.save_model([]) == W.write_map({}, [])
        for p in range(P):
            assert agg.save_partition(p) == W.write_darr(w[p]), p
        assert agg.save_model_list() == W.write_dlist(np.concatenate(w))
        # the chunked call: 16-byte pieces, and a piece size that leaves an odd-sized last piece
        got, offs = _collect(agg, None, 16)
        assert got == whole and offs[:3] == [0, 16, 32][:len(offs)]
        chunk = next(c for c in [*range(1000, 1016), *range(17, 200)] if c < len(whole) and (len(whole) % c) % 2 == 1)
        got, offs = _collect(agg, None, chunk)
        assert got == whole
        with pytest.raises(ipls.IplsError) as e:
            agg.save_model([0, P])
        assert e.value.code == RANGE


@pytest.mark.parametrize("shape,devices", CASES, ids=IDS)
def test_load_sets_blends_and_leaves_the_rest(ipls, O, shape, devices):
    with _open(ipls, shape, devices) as agg:
        P = agg.n_partitions
        g = _weights(agg, 23)
        # the file holds longer arrays than the partitions for odd p: the first L_p values count
        held = {p: (np.concatenate([x, [9.0, -9.0]]) if p & 1 else x) for p, x in enumerate(g)}
        order = list(range(P - 1, -1, -1))
        file = W.write_map(held, order)
        assert agg.LoadSavedModel(file) == P
        for p in range(P):
            _exact(agg.read(p, ipls.TGT_WEIGHTS), g[p], f"SET p{p}")
        # leaving-peer blend on top of known weights
        w0 = [np.linspace(-3.0, 5.0, L) * 1.000000123 for L in agg.lengths]
        _place(agg, w0)
        assert agg.LoadSavedModel(file, leaving_peer=True) == P
        for p in range(P):
            assert_bits_equal(agg.read(p, ipls.TGT_WEIGHTS), O.blend(w0[p], g[p], 0.6, 1 - 0.6), f"BLEND p{p}")
        # a ChangedList: the others stay bit for bit
        _place(agg, w0)
        sub = [P - 1, 1] if P > 2 else [P - 1]
        assert agg.LoadSavedModel(file, sub + sub[:1]) == len(sub)
        for p in range(P):
            _exact(agg.read(p, ipls.TGT_WEIGHTS), g[p] if p in sub else w0[p], f"subset p{p}")
        # an accumulator that is logically zero: SET writes it, BLEND blends with +0.0
        assert agg.LoadSavedModel(file, [0], target=ipls.TGT_AGG) == 1
        _exact(agg.read(0, ipls.TGT_AGG), g[0], "SET into AGG")
        assert agg.LoadSavedModel(file, [0], target=ipls.TGT_REP, leaving_peer=True) == 1
        assert_bits_equal(agg.read(0, ipls.TGT_REP), O.blend(np.zeros(agg.lengths[0]), g[0], 0.6, 1 - 0.6), "BLEND into REP")


@pytest.mark.parametrize("shape,devices", [(("synthetic", 7, 5), None), (("synthetic", TILE + 1, 3), None), (MODEL, None),
                                           (MODEL, [0, 0])], ids=["7x5", "2049x3", "model", "model-2shards"])
def test_errors_leave_every_target_unchanged(ipls, shape, devices):
    with _open(ipls, shape, devices) as agg:
        P = agg.n_partitions
        w0 = _weights(agg, 5)
        _place(agg, w0)
        g = dict(enumerate(_weights(agg, 6)))

        def unchanged(what):
            for p, x in enumerate(_all(agg, ipls)):
                _exact(x, w0[p], f"{what}: partition {p}")

        missing = W.write_map({p: g[p] for p in range(P) if p != 1}, [p for p in range(P) if p != 1])
        for leaving in (False, True):
            with pytest.raises(ipls.IplsError) as e:       # parameters.get(1) == null
                agg.LoadSavedModel(missing, [0, 1], leaving_peer=leaving)
            assert e.value.code == RANGE
            unchanged("missing key")
        short = dict(g)
        short[P - 1] = g[P - 1][:-1]
        with pytest.raises(ipls.IplsError) as e:           # ArrayIndexOutOfBounds, Updater.java:67
            agg.LoadSavedModel(W.write_map(short, range(P)))
        assert e.value.code == RANGE
        unchanged("short array")
        with pytest.raises(ipls.IplsError) as e:           # a key that is no partition
            agg.LoadSavedModel(W.write_map({0: g[0], P: g[0]}, [0, P]))
        assert e.value.code == RANGE
        unchanged("foreign key")
        with pytest.raises(ipls.IplsError) as e:
            agg.LoadSavedModel(W.write_map(g, range(P))[:-3])
        assert e.value.code == FORMAT
        unchanged("truncated file")
        # a DLIST with one corrupted record byte: only the device sees it
        M = agg.flat_size
        model = W.edge_values(M + 3, 8)
        lst = bytearray(W.write_dlist(model))
        for rec in sorted({1, M // 2, M - 1, M + 2} - {0}):
            bad = bytearray(lst)
            bad[129 + 14 * rec - 6 + 3] ^= 0x10
            with pytest.raises(ipls.IplsError) as e:
                agg.InitializeWeights(bytes(bad), java_list=True)
            assert e.value.code == FORMAT, rec
            unchanged(f"corrupted record {rec}")
        with pytest.raises(ipls.IplsError) as e:           # fewer values than the model
            agg.InitializeWeights(W.write_dlist(model[:M - 1]), java_list=True)
        assert e.value.code == RANGE
        unchanged("short list")


@pytest.mark.parametrize("shape,devices", [(("synthetic", 7, 5), None), (("synthetic", TILE + 1, 3), None), (MODEL, None),
                                           (MODEL, [0, 0])], ids=["7x5", "2049x3", "model", "model-2shards"])
def test_model_list_initialises_like_the_plain_model(ipls, shape, devices):
    """InitializeWeights from the serialised ArrayList<Double> leaves what
    InitializeWeights(values) leaves -- after doubleToLongBits: NaN canonical."""
    with _open(ipls, shape, devices) as a, _open(ipls, shape, devices) as b:
        M = a.flat_size
        model = W.edge_values(M + 2, 31)
        a.InitializeWeights(W.write_dlist(model), java_list=True)
        b.InitializeWeights(np.frombuffer(W.canon_be(model), dtype=">f8").astype(np.float64).copy())
        for p in range(a.n_partitions):
            for tgt in (ipls.TGT_WEIGHTS, ipls.TGT_AGG, ipls.TGT_REP):
                _exact(a.read(p, tgt), b.read(p, tgt), f"partition {p} target {tgt}")
        _exact(np.concatenate([x[:-1] for x in _all(a, ipls)])[:M],
               np.frombuffer(W.canon_be(model[:M]), dtype=">f8").astype(np.float64), "the model's values")


def test_darr_source_kind(ipls, O):
    """IPLS_HOST_DARR through accumulate, set_weights and blend, like the
    Pair's double[]: a longer array gives its first L_p values to the fold and
    the blend, set_weights keeps GetParameters' rule."""
    from ipls import _native as N
    L = TILE + 5
    with ipls.Aggregator(n_partitions=2, bucket_len=L) as agg:
        g = W.edge_values(L + 2, 3)
        g[np.isnan(g)] = 1.25
        file = np.frombuffer(W.write_darr(g), dtype=np.uint8)
        lib, h = N.lib(), agg.handle
        w0 = np.linspace(1.0, 2.0, L)
        agg.cache_partition(1, w0)
        assert lib.ipls_agg_blend(h, 1, N.TGT_WEIGHTS, file.ctypes.data, file.size, N.HOST_DARR, 0.6, 1 - 0.6) == 0
        assert_bits_equal(agg.read(1, ipls.TGT_WEIGHTS), O.blend(w0, g, 0.6, 1 - 0.6), "blend")
        assert lib.ipls_agg_accumulate(h, 0, N.TGT_AGG, file.ctypes.data, file.size, N.HOST_DARR) == 0
        assert lib.ipls_agg_accumulate(h, 0, N.TGT_AGG, file.ctypes.data, file.size, N.HOST_DARR) == 0
        assert_bits_equal(agg.read(0, ipls.TGT_AGG), (0.0 + g[:L]) + g[:L], "accumulate")
        assert lib.ipls_agg_set_weights(h, 0, file.ctypes.data, file.size, N.HOST_DARR) == RANGE   # longer than L_p
        short = np.frombuffer(W.write_darr(g[:L - 3]), dtype=np.uint8)
        assert lib.ipls_agg_set_weights(h, 0, short.ctypes.data, short.size, N.HOST_DARR) == 0
        assert_bits_equal(agg.read(0, ipls.TGT_WEIGHTS)[:L - 3], g[:L - 3], "set_weights")
        assert lib.ipls_agg_accumulate(h, 0, N.TGT_AGG, short.ctypes.data, short.size, N.HOST_DARR) == RANGE
        assert lib.ipls_agg_accumulate(h, 0, N.TGT_AGG, file.ctypes.data, file.size - 1, N.HOST_DARR) == FORMAT


def test_sink_can_stop_the_delivery(ipls):
    with ipls.Aggregator(n_partitions=3, bucket_len=40) as agg:
        seen = []

        def sink(ptr, off, cnt):
            seen.append(off)
            return len(seen) < 3
        with pytest.raises(ipls.IplsError) as e:
            agg.save_model(sink=sink, chunk_bytes=64)
        assert e.value.code == -1 and seen == [0, 64, 128]
        assert len(agg.save_model()) == 181 + 320 + 2 * 340 + 1      # and the handle goes on


def test_cpp_host_mirror_saved_model(ipls, O, tmp_path):
    """IPLS::save_model / save_partition / Model_list / DownloadMapParameters /
    InitializeWeights_from_list and Updater::_Update_from_leaving_peer of
    host/ipls_host.hpp, through tests/cpp/host_saved_model_driver.cpp."""
    exe = ROOT / "tests" / "cpp" / "build" / "host_saved_model_driver"
    exe.parent.mkdir(parents=True, exist_ok=True)
    lib = ROOT / "ipls-java-api_amd" / "lib"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'ipls-java-api_amd' / 'host'}", str(ROOT / "tests" / "cpp" / "host_saved_model_driver.cpp"),
                    f"-L{lib}", "-lipls_agg", f"-Wl,-rpath,{lib}", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host saved model ok" in r.stdout, r.stdout + r.stderr
    with ipls.Aggregator(30011, 3) as agg:
        lens = agg.lengths
    w = {p: p + 0.5 * np.arange(L) for p, L in enumerate(lens)}
    w0 = {p: 1.0 - 0.25 * np.arange(L) for p, L in enumerate(lens)}
    assert (tmp_path / "leaving_map.ser").read_bytes() == W.write_map(w, [2, 0, 1])
    assert (tmp_path / "leaving_p1.ser").read_bytes() == W.write_darr(w[1])
    flat = np.concatenate([w[p] for p in range(3)])
    assert (tmp_path / "leaving_list.ser").read_bytes() == W.write_dlist(flat)
    blended = {p: O.blend(w0[p], w[p], 0.6, 1 - 0.6) for p in range(3)}    # {2, 0} by the map, 1 by the double[] file
    assert (tmp_path / "taking_map.ser").read_bytes() == W.write_map(blended, [0, 1, 2])
    # InitializeWeights(List<Double>): the first M values, count slots 0.0 (IPLS.java:1880-1901)
    obj, end = J.read_object((tmp_path / "taking_after_list.ser").read_bytes())
    vals = obj["annotations"]["java.util.HashMap"][2::2]
    got = np.concatenate([v["values"][:-1] for v in vals])
    _exact(got, flat[:30011], "model from the list")
    assert all(v["values"][-1] == 0.0 for v in vals)
