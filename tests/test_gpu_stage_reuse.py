"""One stage of the chunked calls (csrc/stage.hpp) reused by every kind of
call in turn, stopped and completed: the order-of-reuse cases its protocol
exists for.  One handle and one thread, so the engine's pool holds exactly one
stage and every call below takes the one the previous call gave back -- after a
give-up (a source or sink that stopped) as after a success, inbound after
outbound, a smaller element after a larger one, a larger buffer after a
smaller one.

Geometry: model size 211, P = 3 (partition arrays of 72, 72 and 70 doubles).
With chunk = 4 a partition is 18 chunks, more than twice the largest ring
(4 slots), the last partition with a short last chunk.  Every result is
compared bit for bit with the oracle (and the restated saved-model writer),
never with the library itself.  Every stop is a callback returning non-zero,
which the API defines.

The ring's shape is read when a stage is first made, so the sequence runs once
with the defaults (3 slots, 2 copy streams) and once in a fresh process with
IPLS_STAGE_SLOTS=2 IPLS_STAGE_STREAMS=1: this file run as a script.
"""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
M, P, CHUNK = 211, 3, 4
INVAL = -1


def _same(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64)), what


def _source(raw, esize, stop_at=None):
    """A chunk source over the contiguous array `raw` (esize bytes per value); stops at its call number stop_at."""
    calls = []

    def src(dst, off, cnt):
        calls.append(off)
        if stop_at is not None and len(calls) - 1 == stop_at:
            return False
        ctypes.memmove(dst, raw.ctypes.data + off * esize, cnt * esize)
        return True
    return src, calls


def _sink(esize=1, stop_at=None):
    """A sink collecting esize * count bytes per call; stops at its call number stop_at."""
    got, calls = bytearray(), []

    def sink(ptr, off, cnt):
        calls.append(off)
        if stop_at is not None and len(calls) - 1 == stop_at:
            return False
        got.extend(ctypes.string_at(ptr, cnt * esize))
        return True
    return sink, got, calls


def run_sequence(ipls, O, W):
    rng = np.random.default_rng(211)
    with ipls.Aggregator(M, P) as agg:
        L = agg.lengths
        assert L == [72, 72, 70]
        # the oracle's state; seeded through calls that use no stage
        AGG = [rng.standard_normal(n) for n in L]
        REP = [np.zeros(n) for n in L]
        WT = [rng.standard_normal(n) for n in L]
        for p in range(P):
            WT[p][-1] = 3.0 + p
            agg.Update(AGG[p], p)
            agg.cache_partition(p, WT[p])

        def raises_inval(call):
            try:
                call()
            except ipls.IplsError as e:
                assert e.code == INVAL, e
            else:
                raise AssertionError("the stopped call returned IPLS_OK")

        # 1. a source that stops at chunk 5: IPLS_E_INVAL, the target unchanged
        x = rng.standard_normal(L[0])
        src, calls = _source(x, 8, stop_at=5)
        raises_inval(lambda: agg.UpdateChunked(0, L[0], src, big_endian=False, chunk=CHUNK))
        assert calls == [0, 4, 8, 12, 16, 20]
        _same(agg.read(0), AGG[0], "1: AGG[0] after a stopped source")

        # 2. the same bucket, to the end, as doubles
        src, calls = _source(x, 8)
        agg.UpdateChunked(0, L[0], src, big_endian=False, chunk=CHUNK)
        assert len(calls) == 18
        O.fold(AGG[0], x)
        _same(agg.read(0), AGG[0], "2: AGG[0] after accumulate_chunked (F64)")

        # 3. a half-precision bucket: a smaller element, nothing regrows
        h = rng.standard_normal(L[2]).astype(np.float16)
        src, calls = _source(h, 2)
        agg.UpdateChunked(2, L[2], src, chunk=CHUNK, dtype=np.float16)
        assert len(calls) == 18 and calls[-1] == 68
        O.fold(AGG[2], h.astype(np.float64))
        _same(agg.read(2), AGG[2], "3: AGG[2] after accumulate_chunked_narrow (f16)")

        # 4. finalize with a sink that stops at chunk 2: the round is consumed all the same
        sink, got, calls = _sink(8, stop_at=2)
        raises_inval(lambda: agg.AggregatePartitionChunked(0, sink, big_endian=False, chunk=CHUNK))
        assert calls == [0, 4, 8]
        wa = np.empty(L[0])
        O.aggregate_partition(AGG[0], REP[0], WT[0], wa)
        _same(np.frombuffer(bytes(got)), WT[0][:8], "4: the chunks delivered before the stop")
        _same(agg.read(0, ipls.TGT_WEIGHTS), WT[0], "4: W[0] after the stopped finalize_chunked")
        _same(agg.read(0), AGG[0], "4: AGG[0] after the stopped finalize_chunked")

        # 5. the whole model: the stage grows from a partition to the segment
        sink, got, calls = _sink(8)
        agg.GetPartitionsChunked(sink, chunk=64)
        assert calls == [0, 64, 128, 192]
        _same(np.frombuffer(bytes(got)), O.get_partitions(WT), "5: get_partitions_chunked")

        # 6. one flat gradient, its chunks straddling both partition boundaries (71, 142)
        flat = rng.standard_normal(M)
        src, calls = _source(flat, 8)
        agg.UpdateGradientChunked(M, src, range(P), big_endian=False, chunk=50)
        assert calls == [0, 50, 100, 150, 200]
        parts = O.organize_gradients(flat, M, P)
        for p in range(P):
            O.fold(AGG[p], parts[p])
            _same(agg.read(p), AGG[p], f"6: AGG[{p}] after update_gradient_chunked")

        # 7. the saved model: a sink that stops on its first piece, then the whole file
        sink, got, calls = _sink(stop_at=0)
        raises_inval(lambda: agg.save_model(sink=sink, chunk_bytes=64))
        assert calls == [0]
        sink, got, calls = _sink()
        assert agg.save_model(sink=sink, chunk_bytes=64) is None
        assert bytes(got) == W.write_map(dict(enumerate(WT)), range(P)), "7: save_model_chunked"

        # 8. and inbound once more
        be = rng.standard_normal(L[1])
        src, calls = _source(be.astype(">f8"), 8)
        agg.UpdateChunked(1, L[1], src, chunk=CHUNK)
        O.fold(AGG[1], be)
        _same(agg.read(1), AGG[1], "8: AGG[1] after the last accumulate_chunked")
        for p in range(P):
            _same(agg.read(p, ipls.TGT_WEIGHTS), WT[p], f"8: W[{p}] at the end")


if __name__ == "__main__":
    for path in (ROOT, ROOT / "ipls-java-api_amd", ROOT / "tests"):
        sys.path.insert(0, str(path))
    import ipls
    import saved_model_writer
    from oracle import oracle
    run_sequence(ipls, oracle, saved_model_writer)
    print("stage reuse ok: slots", os.environ.get("IPLS_STAGE_SLOTS"), "streams", os.environ.get("IPLS_STAGE_STREAMS"))
else:
    import pytest

    torch = pytest.importorskip("torch")
    pytestmark = pytest.mark.gpu

    def test_reuse_with_the_default_ring():
        if not torch.cuda.is_available():
            pytest.fail("-m gpu run without a visible GPU")
        import ipls
        import saved_model_writer
        from oracle import oracle   # checker only
        run_sequence(ipls, oracle, saved_model_writer)

    def test_reuse_with_two_slots_and_one_stream():
        if not torch.cuda.is_available():
            pytest.fail("-m gpu run without a visible GPU")
        env = dict(os.environ, IPLS_STAGE_SLOTS="2", IPLS_STAGE_STREAMS="1")
        r = subprocess.run([sys.executable, str(Path(__file__).resolve())], env=env, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0 and "stage reuse ok: slots 2 streams 1" in r.stdout, r.stdout + r.stderr
