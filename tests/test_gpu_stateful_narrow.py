"""A random sequence over the trainer-format (f32 / half / bf16) and
saved-model calls, interleaved with each other and with the f64 calls, replayed
step by step against the model of tests/narrow_sequence.py, bit for bit.

The engine never zeroes an accumulator where Java would: it sets a "logically
+0.0" flag and leaves last round's sums in the arena, so every entry point has
to resolve the flag (a zero-start kernel, materialize(), or a null source) and
clear it after writing.  On a fresh handle a mistake there is invisible; here
every call meets accumulators that earlier steps left flagged over stale sums,
non-zero, or freshly loaded.  tests/test_narrow_sequence.py shows on the CPU
that each committed plan reaches those situations and that nine kinds of flag
mistake would change a value compared here.

Every case uses the reference geometry Aggregator(M, P) (ragged last partition;
the flat-vector and saved-model calls apply).  The launch records of every
fold and fused round are collected; each case must have reached
k_fold1_narrow, k_reduce_narrow and k_round_narrow for both element sizes with
every start mode they take.  A case (a scripted prefix of about 100 steps, then
300 random ones; 150 at the tile geometry) takes 0.3-0.6 s on an MI355X.
"""
import ctypes
import time

import numpy as np
import pytest

import narrow_fmt as F
import narrow_sequence as S
import saved_model_writer as W
from conftest import assert_bits_equal

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ORIGIN = b"QmS"
INVAL = -1           # IPLS_E_INVAL
_SENT = {"f64": 0x5555555555555555, "f32": 0x55555555, "half": 0x5555, "bf16": 0x5555}
_CARRIER = {"f64": "int64", "f32": "int32", "half": "int16", "bf16": "int16"}
_NPBITS = {"f64": np.uint64, "f32": np.uint32, "half": np.uint16, "bf16": np.uint16}


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


def _exact_bits(got, want, fmt, what):
    """Narrow bit patterns: NaN must meet NaN, everything else the same bits."""
    got = np.ascontiguousarray(got).view(_NPBITS[fmt])
    want = np.ascontiguousarray(want).view(_NPBITS[fmt])
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    gn, wn = S.is_nan_bits(got, fmt), S.is_nan_bits(want, fmt)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ"
    bad = np.flatnonzero((got != want) & ~wn)
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[0]}: {got[bad[0]]:#x} != {want[bad[0]]:#x}"


class _DevOut:
    """n values of a format in device memory, ``off`` elements past a 16-B
    boundary, sentinel bands either side."""

    def __init__(self, ipls, n, fmt, off):
        self.n, self.fmt, self.off = n, fmt, off
        self.t = torch.full((n + off + 40,), _SENT[fmt], dtype=getattr(torch, _CARRIER[fmt]), device="cuda")
        torch.cuda.synchronize()
        assert self.t.data_ptr() % 16 == 0
        es = 8 if fmt == "f64" else F.esize(fmt)
        self.buf = ipls.DeviceBuffer(self.t.data_ptr() + es * off, n, dtype=fmt)

    def bits(self):
        h = self.t.cpu().numpy().view(_NPBITS[self.fmt])
        s = _SENT[self.fmt]
        assert np.all(h[:self.off] == s) and np.all(h[self.off + self.n:] == s), "wrote outside the output"
        return h[self.off:self.off + self.n].copy()


class _Runner:
    """The library side of one plan: operands, and one method per op class."""

    def __init__(self, ipls, O, pool, agg):
        self.ipls, self.O, self.pool, self.agg = ipls, O, pool, agg
        self.T = {"agg": ipls.TGT_AGG, "rep": ipls.TGT_REP, "fut": ipls.TGT_FUTURE, "w": ipls.TGT_WEIGHTS}
        self.START = {"zero": ipls.START_ZERO, "accum": ipls.START_ACCUM, "first": ipls.START_FIRST}
        self.d64 = [torch.from_numpy(g).to("cuda") for g in pool.f64]
        self.dbe = [torch.from_numpy(np.frombuffer(O.be_encode(g), dtype=np.uint8).copy()).to("cuda") for g in pool.f64]
        torch.cuda.synchronize()
        self.keep = {}
        self.pin = ipls.PinnedBuffer(max(8 * pool.Lmax, 4 * pool.M) + 64)
        self.files = {}
        self.records = set()

    def close(self):
        self.agg.close()
        self.pin.close()

    # ---- operands ----
    def dev(self, fmt, k, L, off=0):
        if fmt == "f64":
            return self.ipls.DeviceBuffer(int(self.d64[k].data_ptr()), L)
        if fmt == "be":
            return self.ipls.DeviceBuffer(int(self.dbe[k].data_ptr()), L, big_endian=True)
        if (fmt, k, off) not in self.keep:
            self.keep[(fmt, k, off)] = F.dev(self.ipls, torch, self.pool.bits[fmt][k], fmt, off)
        return self.ipls.DeviceBuffer(self.keep[(fmt, k, off)][1].ptr, L, dtype=fmt)

    def pinned(self, bits, fmt):
        n = bits.size
        self.pin.view(F.bits_dtype(fmt))[:n] = bits
        if fmt == "f32":
            return self.pin.view(np.float32)[:n]
        if fmt == "half":
            return self.pin.view(np.float16)[:n]
        return torch.from_numpy(self.pin.view(np.int16)[:n]).view(torch.bfloat16)

    def operand(self, fmt, k, L, form, off):
        if form == "dev":
            return self.dev(fmt, k, L, off)
        if fmt == "f64":
            return self.pool.f64[k][:L]
        if fmt == "be":
            return self.O.be_encode(self.pool.f64[k][:L])
        bits = self.pool.bits[fmt][k][:L]
        return self.pinned(bits, fmt) if form == "pinned" else F.host(torch, bits, fmt)

    def flat(self, s):
        bits = self.pool.flat[s["fmt"]][s["j"]]
        if s["form"] == "dev":
            key = ("flat", s["fmt"], s["j"], s["off"])
            if key not in self.keep:
                self.keep[key] = F.dev(self.ipls, torch, bits, s["fmt"], s["off"])
            return self.keep[key][1]
        return self.pinned(bits, s["fmt"]) if s["form"] == "pinned" else F.host(torch, bits, s["fmt"])

    def record(self, want_kernel=None, what=""):
        li = self.agg.last_launch()
        if want_kernel is not None:
            assert li["kernel"] == want_kernel, f"{what}: {li}"
        self.records.add((li["kernel"], li["start"]))
        return li

    def refused(self, fn, code):
        if code is None:
            fn()
            return None
        with pytest.raises(self.ipls.IplsError) as e:
            fn()
        assert e.value.code == INVAL
        return "INVAL"

    # ---- one step: {name: what the library returned} ----
    def run(self, s, exp):
        ipls, agg, pool, p = self.ipls, self.agg, self.pool, s["p"]
        op, L, what = s["op"], pool.lengths[p], f"step {s['i']} {s['op']}"
        want = {n: (k, v) for n, k, v in exp}
        if op in ("update", "update64"):
            x = self.operand(s["fmt"], s["k"], L, s["form"], s["off"])
            agg.Update(x, p, from_clients=s["tgt"] == "agg", from_future=s["tgt"] == "fut")
            if op == "update":       # aligned and host operands: k_fold1_narrow; off a 16-B boundary: the table route
                li = self.record((F.reduce_kernel if s["off"] else F.fold_kernel)(ipls, s["fmt"]), what)
                assert li["seqf"] == (0 if s["off"] else 1), f"{what}: {li}"
            return {}
        if op == "queue":
            bufs = [(self.dev(f, k, L, off), p) for f, k, off in s["items"]]
            if s["many"]:
                t = agg.UpdateAsyncMany(bufs, from_clients=s["tgt"] == "agg")
            else:
                for b, _ in bufs:
                    t = agg.UpdateAsync(b, p, from_clients=s["tgt"] == "agg")
            agg.Wait(t)
            self.record()
            return {}
        if op == "batch":
            tab = [[self.dev(s["fmt"], k, pool.lengths[p + q], s["off"]) for k in row] for q, row in enumerate(s["rows"])]
            agg.reduce_batch(p, tab, start_mode=self.START[s["mode"]], target=self.T[s["tgt"]])
            li = self.record(F.reduce_kernel(ipls, s["fmt"]), what)
            assert li["seqf"] == (0 if s["off"] else 1), f"{what}: {li}"
            return {}
        if op == "chunked":
            bits, es, calls = pool.bits[s["fmt"]][s["k"]][:L], F.esize(s["fmt"]), []

            def source(dst, off, cnt):
                calls.append(off)
                if len(calls) - 1 == s["stop_at"]:
                    return False
                ctypes.memmove(dst, bits.ctypes.data + es * off, es * cnt)
                return True
            code = self.refused(lambda: agg.UpdateChunked(p, L, source, from_clients=s["tgt"] == "agg", chunk=s["chunk"],
                                                          dtype=F.np_dtype(s["fmt"])), want["code"][1])
            if code is None:
                self.record(F.fold_kernel(ipls, s["fmt"]), what)
            return {"code": code}
        if op == "round":
            how, afmt, off = s["avg"]
            tab = [[self.dev(s["src"], k, pool.lengths[p + q]) for k in row] for q, row in enumerate(s["rows"])]
            if s["misalign"]:
                tab[0][0] = self.dev(s["src"], s["rows"][0][0], L, s["misalign"])
            got = {}
            if how == "none":
                assert agg.aggregate_round(p, tab, with_average=False) is None
            elif how == "dtype":
                r = agg.aggregate_round(p, tab, dtype=np.float64 if afmt == "f64" else F.np_dtype(afmt))
                got["averages"] = r
            else:
                out = _DevOut(ipls, want["averages"][1].size, afmt, off % 2 if afmt == "f64" else off)
                assert agg.aggregate_round(p, tab, out=out.buf) is out.buf
                agg.sync()
                got["averages"] = out.bits().view(np.float64) if afmt == "f64" else out.bits()
            if s["rows"][0]:
                fused = s["src"] in S.NARROW and not s["misalign"] and (how == "none" or afmt in S.NARROW)
                kern = None
                if fused:
                    kern = ipls.KERNEL_ROUND_F32 if s["src"] == "f32" else ipls.KERNEL_ROUND_H16
                elif s["src"] in S.NARROW and not (s["misalign"] and len(agg.devices) > 1):
                    # (each shard decides for its own partitions: one bucket off a 16-B
                    # boundary leaves the other shards' launches fused)
                    kern = F.reduce_kernel(ipls, s["src"])
                self.record(kern, what)
            return got
        if op == "get":
            fmt, n = s["fmt"], agg.flat_size
            if s["how"] == "dtype":
                return {"model": agg.GetPartitions(dtype=F.np_dtype(fmt))}
            if s["how"] == "out":
                out = _DevOut(ipls, n, fmt, s["off"])
                agg.GetPartitions(out=out.buf)
                agg.sync()
                return {"model": out.bits()}
            got = bytearray(n * F.esize(fmt))

            def sink(ptr, off, cnt):
                got[off:off + cnt] = ctypes.string_at(ptr, cnt)
                return True
            agg.GetPartitionsChunked(sink, dtype=F.np_dtype(fmt), chunk=s["chunk"])
            return {"model": np.frombuffer(bytes(got), dtype=F.bits_dtype(fmt))}
        if op == "organize":
            r = agg.OrganizeGradients(self.flat(s))
            return {f"organize[{q}]": r[q] for q in range(agg.n_partitions)}
        if op == "ugrad":
            agg.UpdateGradient(self.flat(s), s["auth"])
            return {}
        if op == "init":
            agg.InitializeWeights(self.flat(s))
            return {}
        if op == "init_dlist":
            if ("dlist", s["j"]) not in self.files:
                self.files[("dlist", s["j"])] = W.write_dlist(pool.dlist[s["j"]])
            agg.InitializeWeights(self.files[("dlist", s["j"])], java_list=True)
            return {}
        if op == "save_model":
            return {"file": agg.save_model(s["auth"], target=self.T[s["tgt"]])}
        if op == "save_sink":
            got = bytearray()

            def fsink(ptr, off, cnt):
                assert off == len(got) and 0 < cnt <= s["chunk_bytes"]
                got.extend(ctypes.string_at(ptr, cnt))
                return True
            assert agg.save_model(s["auth"], sink=fsink, target=self.T[s["tgt"]], chunk_bytes=s["chunk_bytes"]) is None
            return {"file": bytes(got)}
        if op == "save_partition":
            return {"file": agg.save_partition(p, target=self.T[s["tgt"]])}
        if op == "save_list":
            return {"file": agg.save_model_list(target=self.T[s["tgt"]])}
        if op == "publish":
            return {"text": agg.publish_partial(p, s["a"], s["b"], origin=ORIGIN, target=self.T[s["tgt"]])}
        if op == "load":
            key = ("map", tuple(sorted(s["held"].items())), tuple(s["order"]))
            if key not in self.files:
                self.files[key] = W.write_map(pool.file_arrays(s["held"]), s["order"])
            return {"done": agg.LoadSavedModel(self.files[key], s["parts"], leaving_peer=s["leaving"], target=self.T[s["tgt"]])}
        if op == "aggpart":
            agg.AggregatePartition(p)
        elif op == "reset":
            agg.reset() if s["all"] else agg.reset(p)
        elif op == "promote":
            agg.PromoteFuture(s["qs"])
        elif op == "cache":
            agg.cache_partition(p, self.O.be_encode(pool.f64[s["k"]][:s["n"]]))
        elif op == "refuse":
            d = self.dev(s["fmt"], s["k"], L)
            if s["which"] == "mixed":
                # one dtype per table: the Python front refuses the mix before any library call
                # (the C-ABI takes one kind per table, so a mix cannot reach it)
                with pytest.raises(ValueError, match="one dtype"):
                    agg.reduce_batch(p, [[d, self.dev(s["fmt2"], s["k2"], L)]])
                return {"code": "INVAL"}
            call = {"cache": lambda: agg.cache_partition(p, d), "areplica": lambda: agg.UpdateAsyncReplica(d, p),
                    "leaving": lambda: agg.UpdateLeavingPeer(d, p), "other": lambda: agg.OtherReplicaGradients(p, 1, d)}
            return {"code": self.refused(call[s["which"]], "INVAL")}
        else:
            assert op == "read", op
        return {}

    def compare(self, s, exp, got):
        O, agg = self.O, self.agg
        for name, kind, want in exp:
            what = f"step {s['i']} {s['op']} (p{s['p']}): {name}"
            if name not in got and kind == "f64":            # a read of the state
                if name == "GetPartitions":
                    g = agg.GetPartitions()
                else:
                    t, q = name[:-1].split("[")
                    g = agg.read(int(q), self.T[t])
            else:
                g = got[name]
            if kind == "f64":
                assert_bits_equal(g, want, what)
            elif kind in S.NARROW:
                _exact_bits(g, want, kind, what)
            elif kind == "map":
                assert g == W.write_map(*want), what
            elif kind == "darr":
                assert g == W.write_darr(want), what
            elif kind == "dlist":
                assert g == W.write_dlist(want), what
            elif kind == "frame":
                assert g == O.java_b64url_encode(O.frame_encode(want[0], want[1], want[2], 3, ORIGIN)), what
            else:
                assert g == want, what


def required_records(ipls):
    """(kernel, start) of the launch records every case must reach."""
    Z, A, Fi = ipls.START_ZERO, ipls.START_ACCUM, ipls.START_FIRST
    return ({(k, st) for k in (ipls.KERNEL_FOLD1_F32, ipls.KERNEL_FOLD1_H16, ipls.KERNEL_ROUND_F32, ipls.KERNEL_ROUND_H16)
             for st in (Z, A)}
            | {(k, st) for k in (ipls.KERNEL_REDUCE_F32, ipls.KERNEL_REDUCE_H16) for st in (Z, A, Fi)})


def run_plan(ipls, O, seed, geom, steps, group=1, devices=None, secure=False, *, with_prefix=True):
    """Replay plan(seed, geometry) against a handle and the model; returns the
    set of (kernel, start) launch records reached."""
    M, P = S.GEOMETRIES[geom]
    lengths, offsets = S.geometry(M, P)
    pool = S.Pool(seed, lengths, offsets)
    model = S.Model(pool, secure=secure)
    agg = ipls.Aggregator(M, P, devices=devices, secure=secure)
    r = _Runner(ipls, O, pool, agg)
    try:
        assert agg.lengths == lengths and agg.offsets == offsets and agg.flat_size == pool.M
        agg.set_coalesce(group)
        for s in S.plan(seed, lengths, offsets, steps, with_prefix=with_prefix):
            exp = model.apply(s)
            r.compare(s, exp, r.run(s, exp))
        r.compare({"i": "end", "op": "read", "p": 0}, model.final(), {})
    finally:
        r.close()
    return r.records


@pytest.mark.parametrize("seed,geom,steps,group,devices,secure", S.CASES, ids=S.CASE_IDS)
def test_stateful_narrow_sequence(ipls, O, seed, geom, steps, group, devices, secure):
    if geom == "tile":          # the committed geometry is built on the tile the launch record reports
        x = np.full(9, F.ONE["half"], dtype=np.uint16)
        keep, buf = F.dev(ipls, torch, x, "half")
        with ipls.Aggregator(n_partitions=1, bucket_len=9) as a:
            a.reduce_batch(0, [[buf]])
            li = a.last_launch()
        assert li["kernel"] == ipls.KERNEL_REDUCE_H16
        assert (li["block"] * 4 * li["vectors"], li["block"]) == (S.TILE16, S.BLOCK16), li
    t0 = time.perf_counter()
    records = run_plan(ipls, O, seed, geom, steps, group, devices, secure)
    print(f"stateful narrow sequence seed {seed} {geom}: {time.perf_counter() - t0:.2f} s")
    missing = required_records(ipls) - records
    assert not missing, f"launch records never reached: {sorted(missing)} (reached {sorted(records)})"
