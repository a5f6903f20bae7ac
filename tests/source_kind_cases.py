"""The (entry point, operand kind) matrix of tests/test_gpu_source_kinds.py:
the cases, generated deterministically, and the rig that runs one -- shared
with tests/golden/make_source_kind_codes.py, which records each case's return
code and error text in tests/golden/source_kind_codes.txt.

The handle is tiny: a model of 37 values in 3 partitions (lengths 14, 14, 12)
on one shard.  Every entry point that takes (src, n, src_kind) meets every
kind 0..17 (17 is no kind) with n one short of, at and one past its length,
from pageable and pinned host memory or from device memory at element offsets
0 and 1; the trainer kinds also one byte off their alignment, the container
kinds also cut by a byte, a frame also empty.  A source is
always memory of the space its kind names, and a device pointer is only ever
misaligned where every call checks it (the trainer kinds) -- a pointer the
library does not refuse would be read by a kernel.

The zero-copy seam has handles of its own: one partition of 8,192 doubles
(exactly the 65,536 bytes from which accumulate reads a pinned bucket in
place) and one of 8,191.
"""
import ctypes
import zlib
from collections import namedtuple

import numpy as np

import narrow_fmt as F
import saved_model_writer as SW

M, P, PART = 37, 3, 1            # the calls on one partition use partition 1 (14 values)
AGG, REP, WEIGHTS, FUT = 0, 1, 2, 4
TARGETS = (AGG, REP, WEIGHTS, FUT)
HOST_F64, HOST_BE, HOST_FRAME, DEV_F64, DEV_BE, HOST_PAIR, HOST_DARR = 0, 1, 2, 3, 4, 6, 9
KINDS = tuple(range(18))
DEV_KINDS = (3, 4, 8, 11, 13, 15)           # DEV_TEXT (8) is an output kind, but it names device memory
TRAINER = {11: "f32", 12: "f32", 13: "half", 14: "half", 15: "bf16", 16: "bf16"}
BOXED = (HOST_FRAME, HOST_PAIR, HOST_DARR)  # n is the byte length
BLEND_A, BLEND_B = 0.5, 2.0
AGGREGATOR = 7
SPLIT_PART, OWNED = 2, (0, 2)
CHUNK = 8

# entry point -> the accumulator it writes (None: see the test)
CALLS = {
    "accumulate": AGG, "accumulate_async": REP, "accumulate_range": FUT, "set_weights": WEIGHTS, "blend": REP,
    "other_replica": REP, "other_replica_first": REP, "load_model": None, "split": None, "update_gradient": AGG,
    "update_indirect": AGG, "accumulate_chunked": AGG, "accumulate_chunked_narrow": REP,
}
FLAT_CALLS = ("load_model", "split", "update_gradient")     # n counts the flat vector
SEAM_LENS = (8192, 8191)

Case = namedtuple("Case", "id call kind dn mem")


def esize(kind):
    return F.esize(TRAINER[kind]) if kind in TRAINER else 8


def mems(kind):
    if kind in DEV_KINDS:
        return ("dev+0", "dev+1") + (("dev+odd",) if kind in TRAINER else ())
    more = ("pageable+odd",) if kind in TRAINER else ("pageable-cut",) if kind in BOXED else ()   # cut: the last byte missing
    return ("pageable", "pinned") + more + (("pageable-empty",) if kind == HOST_FRAME else ())       # empty: array length 0


def cases(call):
    out = []
    if call == "update_indirect":        # no kind argument: the bytes of a GetParameters file
        grid = [(-1, m) for m in ("pageable", "pinned")]
    elif call.startswith("accumulate_chunked"):
        grid = [(k, "source") for k in KINDS]
    else:
        grid = [(k, m) for k in KINDS for m in mems(k)]
    for kind, mem in grid:
        for dn in (-1, 0, 1):
            out.append(Case(f"{call}/k{kind}/n{dn:+d}/{mem}", call, kind, dn, mem))
    return out


def seam_cases():
    out = []
    for L in SEAM_LENS:
        for call in ("accumulate", "accumulate_async"):
            for kind in (HOST_F64, HOST_BE):
                for n in (8191, 8192):
                    for off in (0, 8):
                        out.append(Case(f"seam{L}.{call}/k{kind}/n{n}/pinned+{off}", call, kind, n - L, f"pinned+{off}"))
    return out


def all_cases():
    return [c for call in CALLS for c in cases(call)] + seam_cases()


def load_codes(path):
    """id -> (return code, error text) of the recording."""
    out = {}
    for line in path.read_text().splitlines():
        cid, rc, text = line.split("\t")
        out[cid] = (int(rc), text)
    return out


def payload(kind, count, seed):
    """`count` values of the kind: (bytes, the doubles a reader of the kind gets, the call's n)."""
    from oracle import oracle as O, javaser as J   # checker only: the reference's own encoders
    rng = np.random.default_rng(seed)
    count = max(count, 0)
    if kind in TRAINER:
        bits = F.from_f32(rng.standard_normal(count).astype(np.float32), TRAINER[kind])
        return np.ascontiguousarray(bits).view(np.uint8), F.widen(bits, TRAINER[kind]), count
    vals = rng.standard_normal(count)
    if kind in (HOST_BE, DEV_BE):
        raw = vals.astype(">f8").tobytes()
    elif kind == HOST_FRAME:
        raw = O.frame_encode(vals, PART, 9, 3, b"")
    elif kind == HOST_PAIR:
        raw = J.encode_pair(4, vals)
    elif kind == HOST_DARR:
        raw = SW.write_darr(vals)
    else:
        raw = vals.tobytes()
    return np.frombuffer(raw, dtype=np.uint8), vals, len(raw) if kind in BOXED else count


Result = namedtuple("Result", "rc text vals n out")


class Rig:
    """One handle in a known state, and the calls on it.  prepare() leaves, in
    every partition, AGG and FUT logically zero over stale non-zero memory, REP
    holding values and W holding values; probe() folds -0.0 into AGG, REP and
    FUT, which leaves values as they are and turns a logically-zero accumulator
    into +0.0 -- so a zero flag that a call cleared shows its stale memory, and
    one that a call set hides values."""

    def __init__(self, ipls, torch, model_size=M, n_partitions=P, bucket_len=0):
        from ipls import _native as N
        self.N, self.torch, self.ipls = N, torch, ipls
        self.agg = ipls.Aggregator(model_size, n_partitions, bucket_len=bucket_len)
        self.lib, self.h = N.lib(), self.agg._h
        self.lengths = list(self.agg.lengths)
        self.P = n_partitions
        rng = np.random.default_rng(20261020)
        self.w0, self.a, self.b, self.c = ([rng.standard_normal(L) for L in self.lengths] for _ in range(4))
        self.negzero = [np.full(L, -0.0) for L in self.lengths]

    def close(self):
        self.agg.close()

    # ---- plain calls that must succeed ----
    def ok(self, rc):
        assert rc >= 0, (rc, self.N.last_error(None))
        return rc

    def fold(self, p, target, values):
        v = np.ascontiguousarray(values, dtype=np.float64)
        self.ok(self.lib.ipls_agg_accumulate(self.h, p, target, v.ctypes.data, v.size, HOST_F64))

    def read(self, p, target):
        out = np.empty(self.lengths[p])
        self.ok(self.lib.ipls_agg_read(self.h, p, target, out.ctypes.data, out.size, HOST_F64))
        return out

    def prepare(self):
        for p in range(self.P):
            self.ok(self.lib.ipls_agg_set_weights(self.h, p, self.w0[p].ctypes.data, self.lengths[p], HOST_F64))
            self.fold(p, AGG, self.a[p])
            self.ok(self.lib.ipls_agg_promote_future(self.h, (ctypes.c_int32 * 1)(p), 1))   # FUT: zero over a (+ ...)
            self.fold(p, AGG, self.b[p])
            self.ok(self.lib.ipls_agg_reset(self.h, p))                                      # AGG, REP: zero over values
            self.fold(p, REP, self.c[p])

    def model(self):
        """The prepared state as values: {(p, target): array}."""
        st = {}
        for p in range(self.P):
            st[p, AGG], st[p, FUT] = np.zeros(self.lengths[p]), np.zeros(self.lengths[p])
            st[p, REP], st[p, WEIGHTS] = self.c[p].copy(), self.w0[p].copy()
        return st

    def probe(self):
        for p in range(self.P):
            for t in (AGG, REP, FUT):
                self.fold(p, t, self.negzero[p])

    def state(self):
        return {(p, t): self.read(p, t) for p in range(self.P) for t in TARGETS}

    # ---- memory ----
    def place(self, raw, mem, kind):
        """(keepalive, address) of the bytes in the memory `mem` names."""
        pad = 96
        place, _, shift = mem.partition("+")
        if shift in ("", "odd"):
            off = 1 if shift else 0
        else:
            off = int(shift) * (esize(kind) if place == "dev" else 1)   # elements of device memory, bytes of host memory
        if place == "dev":
            t = self.torch.zeros(raw.size + pad, dtype=self.torch.uint8, device="cuda")
            assert t.data_ptr() % 16 == 0
            if raw.size:
                t[off:off + raw.size] = self.torch.from_numpy(raw.copy()).cuda()
            self.torch.cuda.synchronize()
            return t, t.data_ptr() + off
        if place == "pinned":
            b = self.ipls.PinnedBuffer(raw.size + pad)
            assert b.ptr % 16 == 0
            b.view()[off:off + raw.size] = raw
            return b, b.ptr + off
        a = np.zeros(raw.size + pad + 16, dtype=np.uint8)
        base = (-a.ctypes.data) % 16
        a[base + off:base + off + raw.size] = raw
        return a, a.ctypes.data + base + off

    # ---- one case ----
    def run(self, case):
        seed = zlib.crc32(case.id.encode())
        lib, h, N = self.lib, self.h, self.N
        call = case.call
        if call in FLAT_CALLS:
            count = M + case.dn
        else:
            count = self.lengths[PART if self.P > 1 else 0] + case.dn
        kind = HOST_BE if call == "update_indirect" else case.kind
        raw, vals, n = payload(kind, 0 if case.mem == "pageable-empty" else count, seed)
        if case.mem == "pageable-cut":
            raw, n = raw[:-1], n - 1
        keep, ptr, out = None, None, None
        if case.mem != "source":
            keep, ptr = self.place(raw, case.mem, kind)
        part = PART if self.P > 1 else 0
        target = CALLS[call] if self.P > 1 else AGG
        ticket = ctypes.c_uint64(0)
        if call == "accumulate":
            rc = lib.ipls_agg_accumulate(h, part, target, ptr, n, kind)
        elif call == "accumulate_async":
            rc = lib.ipls_agg_accumulate_async(h, part, target, ptr, n, kind, ctypes.byref(ticket))
        elif call == "accumulate_range":
            rc = lib.ipls_agg_accumulate_range(h, part, target, ptr, 0, n, kind, ctypes.byref(ticket))
        elif call == "set_weights":
            rc = lib.ipls_agg_set_weights(h, part, ptr, n, kind)
        elif call == "blend":
            rc = lib.ipls_agg_blend(h, part, target, ptr, n, kind, BLEND_A, BLEND_B)
        elif call in ("other_replica", "other_replica_first"):
            if call == "other_replica":      # something stored to measure the download against
                self.ok(lib.ipls_agg_other_replica(h, part, AGGREGATOR, self.a[part].ctypes.data, self.a[part].size, HOST_F64))
            rc = lib.ipls_agg_other_replica(h, part, AGGREGATOR, ptr, n, kind)
        elif call == "load_model":
            rc = lib.ipls_agg_load_model(h, ptr, n, kind)
        elif call == "split":
            out = np.full(self.lengths[SPLIT_PART], np.nan)
            rc = lib.ipls_agg_split(h, ptr, n, kind, SPLIT_PART, out.ctypes.data, HOST_F64)
        elif call == "update_gradient":
            rc = lib.ipls_agg_update_gradient(h, ptr, n, kind, (ctypes.c_int32 * len(OWNED))(*OWNED), len(OWNED))
        elif call == "update_indirect":
            rc = lib.ipls_agg_update_indirect(h, part, target, ptr, raw.size)
        else:
            s = esize(kind)

            @N.CHUNK_SOURCE
            def source(_ctx, dst, off, cnt):
                ctypes.memmove(dst, raw.ctypes.data + off * s, cnt * s)
                return 0
            fn = lib.ipls_agg_accumulate_chunked if call == "accumulate_chunked" else lib.ipls_agg_accumulate_chunked_narrow
            rc = fn(h, part, target, n, kind, CHUNK, source, None)
        text = N.last_error(None) if rc < 0 else ""
        if rc >= 0 and call in ("accumulate_async", "accumulate_range"):
            self.ok(lib.ipls_agg_wait(h, ticket.value))
        self.ok(lib.ipls_agg_sync(h))      # nothing reads the source after this
        del keep
        return Result(rc, text, vals, n, out)

    def finish(self, case):
        """After a case: Collect_Replicas where the case stored something, so that the
        store shows in REP and is empty again (an array longer than the partition
        stays, and is dropped); then the probe.  Returns Collect_Replicas' result."""
        rc = None
        if case.call.startswith("other_replica"):
            rc = self.lib.ipls_agg_collect_replicas(self.h, None)
            if rc < 0:
                self.ok(self.lib.ipls_agg_other_replica_drop(self.h, PART, AGGREGATOR))
        self.probe()
        return rc
