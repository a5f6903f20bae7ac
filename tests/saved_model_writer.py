"""What a JDK 8 ObjectOutputStream writes for the three saved-model objects of
IPLS, restated from the Java Object Serialization grammar on the oracle's
stream writer (oracle.javaser._W).  TEST INFRASTRUCTURE ONLY: the checker of
ipls_saved_* / ipls_darr_* / ipls_dlist_* and of the save_* / load_saved calls
(tests/test_saved_model.py, tests/test_gpu_saved_model.py).  Nothing here
calls the library.

  HashMap<Integer,double[]>  IPLS.save_model                    IPLS.java:1904-1911
  double[]                   MyIPFSClass._Upload_File(double[]) MyIPFSClass.java:261-270
  ArrayList<Double>          `<ID>Model` / `<ID>ETHModel`       IPLS.java:547-558, 2255-2273
"""
import numpy as np

from oracle import javaser as J

SUID_HASHMAP = 0x0507DAC1C31660D1      # JDK 8 java.util.HashMap (source; no reference file holds one)
SUID_ARRAYLIST = 0x7881D21D99C7619D    # the reference's Uniform/Node1
SUID_DOUBLE = 0x80B3C24A296BFB04       # the reference's Uniform/Node1
CANON_NAN = 0x7FF8000000000000


def _desc(w, name, suid, flags, fields, sup=None):
    """TC_CLASSDESC name suid flags fields TC_ENDBLOCKDATA super -> the descriptor's handle."""
    w.u8(J.TC_CLASSDESC); w.utf(name); w.u64(suid); h = w.handle()
    w.u8(flags); w.u16(len(fields))
    for t, fname in fields:
        w.u8(ord(t)); w.utf(fname)
    w.u8(J.TC_ENDBLOCKDATA)
    if sup is None:
        w.u8(J.TC_NULL)
    else:
        sup()
    return h


def raw_be(values) -> bytes:
    """ObjectOutputStream.writeDoubles: the bits of every double, big-endian (NaN payloads kept)."""
    return np.ascontiguousarray(values, dtype=np.float64).view(np.uint64).astype(">u8").tobytes()


def canon_be(values) -> bytes:
    """Double.doubleToLongBits per value: every NaN becomes 0x7ff8000000000000."""
    v = np.ascontiguousarray(values, dtype=np.float64)
    b = v.view(np.uint64).copy()
    b[np.isnan(v)] = CANON_NAN
    return b.astype(">u8").tobytes()


def hashmap_layout(keys):
    """(iteration order, table size, threshold) of a java.util.HashMap after
    put(k, ..) for k in keys, Integer keys: hash = k ^ (k >>> 16), bin = hash &
    (n - 1); the table starts at 16 and doubles when ++size > 0.75 n; a split
    keeps the relative order of a bin's nodes, so iteration is by bin, then by
    insertion.  (No bin reaches 8 nodes in these tests: no tree bins.)  An
    empty map was never allocated: capacity() 16, threshold 0."""
    ins = []
    cap = 16
    for k in keys:
        if k not in ins:
            ins.append(k)
            if len(ins) > cap * 3 // 4:
                cap *= 2
    if not ins:
        return [], 16, 0

    def bin_of(k):
        u = k & 0xFFFFFFFF
        return (u ^ (u >> 16)) & (cap - 1)
    return sorted(ins, key=lambda k: (bin_of(k), ins.index(k))), cap, cap * 3 // 4


def write_map(weights: dict, put_order) -> bytes:
    """writeObject(map) after map.put(p, weights[p]) for p in put_order."""
    order, cap, thr = hashmap_layout(list(put_order))
    w = J._W()
    w.u8(J.TC_OBJECT)
    _desc(w, "java.util.HashMap", SUID_HASHMAP, J.SC_SERIALIZABLE | J.SC_WRITE_METHOD,
          [("F", "loadFactor"), ("I", "threshold")])
    w.handle()                                   # the map
    w.b += bytes.fromhex("3f400000")             # loadFactor 0.75f
    w.i32(thr)
    w.u8(J.TC_BLOCKDATA); w.u8(8); w.i32(cap); w.i32(len(order))
    h_int = h_dbl = None
    for k in order:
        w.u8(J.TC_OBJECT)
        if h_int is None:
            h_int = _desc(w, "java.lang.Integer", J.SUID["java.lang.Integer"], J.SC_SERIALIZABLE, [("I", "value")],
                          sup=lambda: _desc(w, "java.lang.Number", J.SUID["java.lang.Number"], J.SC_SERIALIZABLE, []))
        else:
            w.ref(h_int)
        w.handle()
        w.i32(k)
        w.u8(J.TC_ARRAY)
        if h_dbl is None:
            h_dbl = _desc(w, "[D", J.SUID["[D"], J.SC_SERIALIZABLE, [])
        else:
            w.ref(h_dbl)
        w.handle()
        a = np.ascontiguousarray(weights[k], dtype=np.float64)
        w.i32(a.size)
        w.b += raw_be(a)
    w.u8(J.TC_ENDBLOCKDATA)
    return bytes(w.b)


def write_darr(values) -> bytes:
    a = np.ascontiguousarray(values, dtype=np.float64)
    w = J._W()
    w.u8(J.TC_ARRAY)
    _desc(w, "[D", J.SUID["[D"], J.SC_SERIALIZABLE, [])
    w.handle()
    w.i32(a.size)
    w.b += raw_be(a)
    return bytes(w.b)


def write_dlist(values) -> bytes:
    a = np.ascontiguousarray(values, dtype=np.float64)
    w = J._W()
    w.u8(J.TC_OBJECT)
    _desc(w, "java.util.ArrayList", SUID_ARRAYLIST, J.SC_SERIALIZABLE | J.SC_WRITE_METHOD, [("I", "size")])
    w.handle()                                   # the list
    w.i32(a.size)
    w.u8(J.TC_BLOCKDATA); w.u8(4); w.i32(a.size)
    body = canon_be(a)
    h_double = None
    for i in range(a.size):
        w.u8(J.TC_OBJECT)
        if h_double is None:
            h_double = _desc(w, "java.lang.Double", SUID_DOUBLE, J.SC_SERIALIZABLE, [("D", "value")],
                             sup=lambda: _desc(w, "java.lang.Number", J.SUID["java.lang.Number"], J.SC_SERIALIZABLE, []))
        else:
            w.ref(h_double)
        w.handle()
        w.b += body[8 * i:8 * i + 8]
    w.u8(J.TC_ENDBLOCKDATA)
    return bytes(w.b)


def edge_values(n: int, seed: int) -> np.ndarray:
    """n doubles whose first ones are the golden edge cases: signed zeros,
    infinities, subnormals, and NaNs with payloads (quiet and signalling)."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n)
    edge = np.array([0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
                     0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x7FF8000000000000, 0x7FF8000000012345,
                     0xFFF8000000000001, 0x7FF0000000000001, 0xFFF4000000000000], dtype=np.uint64).view(np.float64)
    k = min(n, edge.size)
    at = (np.arange(k) * max(1, n // max(k, 1))) % max(n, 1) if n else np.arange(0)
    v[at] = edge[:k]
    return v
