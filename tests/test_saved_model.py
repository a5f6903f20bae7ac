"""Saved-model files on the CPU: the Java-serialised HashMap<Integer,double[]>
(IPLS.save_model, IPLS.java:1904-1911), double[] (MyIPFSClass.java:261-270)
and ArrayList<Double> (IPLS.java:547-558, 2255-2273) host codecs of the C-ABI
(ipls_saved_* / ipls_darr_* / ipls_dlist_*).  The checkers are the oracle's
generic stream reader (oracle.javaser.read_object), the writer restated in
tests/saved_model_writer.py, and a file the reference's own JVM wrote
(tests/golden/ref_uniform_node1.ser, its Uniform/Node1).  No GPU needed."""
import subprocess

import numpy as np
import pytest

import saved_model_writer as W
from conftest import GOLDEN, ROOT
from oracle import javaser as J

NODE1 = (GOLDEN / "ref_uniform_node1.ser").read_bytes()
FORMAT = -6


@pytest.fixture(scope="module")
def ipls():
    import ipls as _ipls
    _ipls.lib()
    return _ipls


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def _read_map(stream: bytes):
    """read_object of a HashMap stream -> (threshold, buckets, size, [(key, values)]), consuming all of it."""
    o, end = J.read_object(stream)
    assert end == len(stream)
    assert o["class"] == "java.util.HashMap"
    assert o["fields"][("java.util.HashMap", "loadFactor")] == 0.75
    ann = o["annotations"]["java.util.HashMap"]
    assert isinstance(ann[0], bytes) and len(ann[0]) == 8
    buckets, size = int.from_bytes(ann[0][:4], "big"), int.from_bytes(ann[0][4:], "big")
    items = ann[1:]
    assert len(items) == 2 * size
    entries = []
    for k, v in zip(items[0::2], items[1::2]):
        assert k["class"] == "java.lang.Integer" and v["kind"] == "array" and v["desc"]["name"] == "[D"
        entries.append((k["fields"][("java.lang.Integer", "value")], v["values"]))
    return o["fields"][("java.util.HashMap", "threshold")], buckets, size, entries


# ---- the reference's own file ----
def test_reference_list_file_parses_and_reencodes(ipls):
    assert len(NODE1) == 824
    o, end = J.read_object(NODE1)
    assert end == 824 and o["class"] == "java.util.ArrayList"
    ref = [x["fields"][("java.lang.Double", "value")] for x in o["annotations"]["java.util.ArrayList"][1:]]
    assert len(ref) == 50 == o["fields"][("java.util.ArrayList", "size")]
    got = ipls.parse_dlist(NODE1)
    assert _bits(got) == _bits(ref)
    assert ipls.encode_dlist(got) == NODE1
    assert W.write_dlist(ref) == NODE1          # the restated writer is pinned by the same file


# ---- MAP against the generic reader and the restated writer ----
@pytest.mark.parametrize("parts,lens", [([0, 1, 2], [5, 5, 4]), ([2, 0], [1, 0]), ([7], [3]),
                                        (list(range(20, 0, -1)), [2] * 20)])
def test_map_reads_back_with_the_generic_reader(ipls, parts, lens):
    w = {p: W.edge_values(n, 100 + p) for p, n in zip(parts, lens)}
    stream = ipls.encode_saved(w, parts)
    order, cap, thr = W.hashmap_layout(parts)
    threshold, buckets, size, entries = _read_map(stream)
    assert (threshold, buckets, size) == (thr, cap, len(parts))
    assert [k for k, _ in entries] == order
    for k, v in entries:
        assert _bits(v) == _bits(w[k])          # raw bits: NaN payloads survive a double[]
    assert stream == W.write_map(w, parts)
    # the layout arithmetic of include/ipls_agg.h
    first = len(w[order[0]])
    assert len(stream) == 181 + 8 * first + sum(20 + 8 * len(w[k]) for k in order[1:]) + 1
    got = ipls.parse_saved(stream)
    assert list(got) == order and all(_bits(got[k]) == _bits(w[k]) for k in order)


EMPTY_MAP = bytes.fromhex("aced0005737200116a6176612e7574696c2e486173684d61700507dac1c31660d103000246000a6c6f6164466163"
                          "746f724900097468726573686f6c6478703f400000000000007708000000100000000078")


@pytest.mark.parametrize("parts,expect,shape", [
    ([3, 19], [3, 19], (16, 12)),
    ([19, 3], [19, 3], (16, 12)),
    ([16, 0], [16, 0], (16, 12)),
    ([16, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 16], (32, 24)),
    ([], [], (16, 0)),
    ([5, 2, 5, 2, 9], [2, 5, 9], (16, 12)),     # listed twice: one key, its first array
])
def test_map_entry_order_is_hashmap_iteration_order(ipls, parts, expect, shape):
    """Literals from the JDK rule (bin = hash & (n - 1), insertion order within a bin, 16 doubling past 0.75 n)."""
    arrays = [np.full(1 + i % 3, float(i)) for i in range(len(parts))]
    w = {}
    for p, a in zip(parts, arrays):
        w.setdefault(p, a)
    stream = ipls.encode_saved(w, parts)
    threshold, buckets, size, entries = _read_map(stream)
    assert [k for k, _ in entries] == expect and size == len(expect)
    assert (buckets, threshold) == shape
    for k, v in entries:
        assert _bits(v) == _bits(w[k])
    if not parts:
        assert stream == EMPTY_MAP and len(stream) == 82


def test_duplicate_listing_keeps_the_first_array(ipls):
    from ipls import _native as N
    import ctypes
    a, b = np.array([1.0, 2.0]), np.array([9.0])
    parts = (ctypes.c_int32 * 2)(4, 4)
    arrs = (ctypes.c_void_p * 2)(a.ctypes.data, b.ctypes.data)
    lens = (ctypes.c_int64 * 2)(2, 1)
    n = N.lib().ipls_saved_encode(parts, 2, arrs, lens, N.HOST_F64, None, 0)
    out = np.empty(n, dtype=np.uint8)
    assert N.lib().ipls_saved_encode(parts, 2, arrs, lens, N.HOST_F64, out.ctypes.data, n) == n
    assert out.tobytes() == W.write_map({4: a}, [4])


# ---- DARR / DLIST layout and round trips ----
@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_round_trips_small_lengths(ipls, n):
    v = W.edge_values(n, n)
    d = ipls.encode_darr(v)
    assert d == W.write_darr(v) and len(d) == 27 + 8 * n
    o, end = J.read_object(d)
    assert end == len(d) and o["desc"]["name"] == "[D" and o["offset"] == 27 and _bits(o["values"]) == _bits(v)
    assert _bits(ipls.parse_darr(d)) == _bits(v)
    m = ipls.encode_saved({1: v, 2: v[:n // 2]}, [1, 2])
    got = ipls.parse_saved(m)
    assert list(got) == [1, 2] and _bits(got[1]) == _bits(v) and _bits(got[2]) == _bits(v[:n // 2])
    lst = ipls.encode_dlist(v)
    assert lst == W.write_dlist(v)
    assert len(lst) == (58 if n == 0 else 129 + 8 + 14 * (n - 1) + 1)
    o, end = J.read_object(lst)
    assert end == len(lst) and o["fields"][("java.util.ArrayList", "size")] == n
    # Double.value goes through doubleToLongBits: NaN canonicalised, everything else bit-exact
    want = np.frombuffer(W.canon_be(v), dtype=">u8").tolist()
    assert _bits(ipls.parse_dlist(lst)) == want


def test_nan_rules(ipls):
    v = np.array([0x7FF8000000012345, 0xFFF0000000000001, 0x7FF4000000000000, 0x8000000000000000],
                 dtype=np.uint64).view(np.float64)
    assert _bits(ipls.parse_darr(ipls.encode_darr(v))) == _bits(v)                     # double[]: raw bits
    assert _bits(ipls.parse_saved(ipls.encode_saved({0: v}))[0]) == _bits(v)
    assert _bits(ipls.parse_dlist(ipls.encode_dlist(v))) == [W.CANON_NAN] * 3 + [0x8000000000000000]


# ---- malformed input ----
def _small_streams(ipls):
    v = np.array([1.5, -2.0, 3.25])
    return {
        "map": ipls.encode_saved({3: v[:2], 19: v}, [3, 19]),
        "map1": ipls.encode_saved({0: v[:1]}),
        "empty": ipls.encode_saved({}),
        "darr": ipls.encode_darr(v),
        "dlist": ipls.encode_dlist(v),
    }


def _parsers(ipls):
    def saved(b):
        return [(k, _bits(a)) for k, a in ipls.parse_saved(b).items()]
    return {"map": saved, "map1": saved, "empty": saved, "darr": lambda b: _bits(ipls.parse_darr(b)),
            "dlist": lambda b: _bits(ipls.parse_dlist(b))}


def test_every_truncation_is_a_format_error(ipls):
    parse = _parsers(ipls)
    for name, good in _small_streams(ipls).items():
        for cut in range(len(good)):
            with pytest.raises(ipls.IplsError) as e:
                parse[name](good[:cut])
            assert e.value.code == FORMAT, (name, cut)
        with pytest.raises(ipls.IplsError) as e:     # and nothing may follow the object
            parse[name](good + b"\x00")
        assert e.value.code == FORMAT


def _framing_positions(name: str, good: bytes, ipls):
    """Byte positions of a small stream that are framing, not data: not an
    array's payload and not a key's int value (another key is another map)."""
    payload = set()
    if name in ("map", "map1"):
        from ipls import _native as N
        import ctypes
        a = np.frombuffer(good, dtype=np.uint8)
        lens, offs = (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 4)()
        n = N.lib().ipls_saved_parse(a.ctypes.data, a.size, None, lens, offs, 4)
        for i in range(n):
            payload.update(range(offs[i], offs[i] + 8 * lens[i]))
            key_at = offs[i] - (23 if i == 0 else 10) - 4       # [key][array framing][length] precede the payload
            payload.update(range(key_at, key_at + 4))
    elif name == "darr":
        payload.update(range(27, len(good)))
    elif name == "dlist":
        n = (len(good) - 129 - 8 - 1) // 14 + 1
        for i in range(n):
            payload.update(range(129 + 14 * i, 129 + 14 * i + 8))
    return [i for i in range(len(good)) if i not in payload]


def test_every_framing_byte_mutation_is_rejected_or_harmless(ipls):
    """A single changed framing byte gives IPLS_E_FORMAT or the very same
    parse, and never a crash."""
    parse = _parsers(ipls)
    rejected = same = 0
    for name, good in _small_streams(ipls).items():
        want = parse[name](good)
        for i in _framing_positions(name, good, ipls):
            for v in {good[i] ^ 0x01, good[i] ^ 0x80, (good[i] + 1) & 0xFF, 0x00, 0xFF, 0x70, 0x78} - {good[i]}:
                b = bytearray(good)
                b[i] = v
                try:
                    got = parse[name](bytes(b))
                except ipls.IplsError as e:
                    assert e.code == FORMAT, (name, i, v)
                    rejected += 1
                else:
                    assert got == want, (name, i, v)
                    same += 1
    assert rejected > 1000 and rejected > 20 * same


def test_parser_rejects_what_the_shape_excludes(ipls):
    v = np.array([1.0, 2.0])
    good = bytearray(ipls.encode_saved({3: v, 19: v}, [3, 19]))
    dup = bytearray(good)
    dup[181 + 16 + 6:181 + 16 + 10] = (3).to_bytes(4, "big")          # second key := the first
    neg = bytearray(good)
    neg[177:181] = (-1).to_bytes(4, "big", signed=True)                # first array length < 0
    big = bytearray(good)
    big[177:181] = (0x7FFFFFFF).to_bytes(4, "big")                     # a length past the stream
    sz = bytearray(good)
    sz[71:75] = (3).to_bytes(4, "big")                                 # one more entry than there is
    for b, why in ((dup, "duplicate key"), (neg, "negative"), (big, "overruns"), (sz, None)):
        with pytest.raises(ipls.IplsError, match=why) as e:
            ipls.parse_saved(bytes(b))
        assert e.value.code == FORMAT
    for stream, parse in ((ipls.encode_darr(v), ipls.parse_dlist), (ipls.encode_dlist(v), ipls.parse_darr),
                          (NODE1, ipls.parse_saved), (bytes(good), ipls.parse_darr)):
        with pytest.raises(ipls.IplsError) as e:
            parse(stream)
        assert e.value.code == FORMAT
    rec = bytearray(ipls.encode_dlist(np.arange(4.0)))
    rec[129 + 8 + 14 + 3] ^= 0x04                                       # a later record's handle
    with pytest.raises(ipls.IplsError, match="element 2") as e:
        ipls.parse_dlist(bytes(rec))
    assert e.value.code == FORMAT


def test_parse_table_is_cut_at_max_entries(ipls):
    import ctypes
    from ipls import _native as N
    stream = ipls.encode_saved({p: np.full(p + 1, 1.0) for p in range(5)})
    a = np.frombuffer(stream, dtype=np.uint8)
    keys = (ctypes.c_int32 * 3)(-1, -1, -1)
    lens, offs = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
    assert N.lib().ipls_saved_parse(a.ctypes.data, a.size, keys, lens, offs, 2) == 5
    assert list(keys) == [0, 1, -1] and list(lens)[:2] == [1, 2] and list(offs)[:2] == [181, 181 + 8 + 20]


# ---- the same corpus under the sanitizers, in a program of its own ----
def test_saved_model_parsers_under_asan():
    """csrc/javaser.cpp built for the host with AddressSanitizer + UBSan and
    fed every truncation and single-byte mutation of small streams of the
    three shapes (tests/cpp/fuzz_saved_model.cpp; no GPU code involved)."""
    out = ROOT / "tests" / "cpp" / "build" / "fuzz_saved_model"
    out.parent.mkdir(parents=True, exist_ok=True)
    csrc = ROOT / "ipls-java-api_amd" / "csrc"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", f"-I{csrc}", str(ROOT / "tests" / "cpp" / "fuzz_saved_model.cpp"),
                    str(csrc / "javaser.cpp"), "-o", str(out)], check=True)
    r = subprocess.run([str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fuzz ok" in r.stdout
