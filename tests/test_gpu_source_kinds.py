"""Every entry point that takes a source operand against every operand kind
(tests/source_kind_cases.py), on the GPU.  Per case:

  * the return code and the error text are those of
    tests/golden/source_kind_codes.txt, recorded from the library as it stood
    before csrc/operand.hpp resolved the sources in one place;
  * an accepted source leaves the bits the oracle computes in the accumulator
    the call writes (for split: in the output), and nothing else changes;
  * a refused one leaves AGG, REP, FUT and W of every partition as they were,
    the "logically zero" flags included: the rig folds -0.0 into every
    accumulator afterwards, which gives +0.0 where the flag still stands and
    the stale memory beneath it where a call cleared it.

Whole states are compared, bit for bit, rather than their checksums.
"""
from pathlib import Path

import numpy as np
import pytest

import source_kind_cases as C

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CODES = C.load_codes(Path(__file__).resolve().parent / "golden" / "source_kind_codes.txt")
RANGE = -2


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


@pytest.fixture(scope="module")
def rig(ipls):
    r = C.Rig(ipls, torch)
    r.prepare()
    r.gbuf = None    # the model of the handle's Gradient_Buff, which outlives a call
    yield r
    r.close()


def test_the_recording_covers_the_matrix():
    assert sorted(CODES) == sorted(c.id for c in C.all_cases())
    # every row of the matrix has sources it takes and sources it refuses
    for call in C.CALLS:
        got = {CODES[c.id][0] < 0 for c in C.cases(call)}
        assert got == {False, True}, call


def _expect(O, rig, case, r, st, collected):
    """Apply the case to the model `st` of the prepared state; returns what else must hold."""
    v, L, p = r.vals, rig.lengths[C.PART], C.PART
    taken = r.rc >= 0 and case.mem != "pageable-empty"    # an empty frame that is not refused is a no-op
    call = case.call
    if call in ("accumulate", "accumulate_chunked", "accumulate_async", "accumulate_chunked_narrow"):
        if taken:
            O.fold(st[p, C.CALLS[call]], v)
    elif call == "accumulate_range":
        if taken:
            st[p, C.FUT][:r.n] = st[p, C.FUT][:r.n] + v[:r.n]
    elif call == "set_weights":
        if taken:   # a frame gives its first L values, GetParameters all it has
            m = L if case.kind == C.HOST_FRAME else v.size
            st[p, C.WEIGHTS][:m] = v[:m]
    elif call == "blend":
        if taken:
            st[p, C.REP] = O.blend(st[p, C.REP], v, C.BLEND_A, C.BLEND_B)
    elif call in ("other_replica", "other_replica_first"):
        stored = rig.a[p].copy() if call == "other_replica" else None
        if taken:
            if stored is None:
                stored = v.copy()
            else:
                stored[:v.size] = stored[:v.size] + v
        if stored is None:
            assert collected == 0, case.id
        elif stored.size > L:    # REP[p] is a double[L]: Collect_Replicas overruns it (IPLS.java:1225)
            assert collected == RANGE, case.id
        else:
            assert collected == 1, case.id
            st[p, C.REP][:stored.size] = st[p, C.REP][:stored.size] + stored
    elif call == "load_model":
        if taken:    # IPLS.java:1883-1895: the values, count slot 0.0; AGG, REP (and FUT) = 0
            c = O.chunk_size(C.M, C.P)
            for q in range(C.P):
                Lq = rig.lengths[q]
                st[q, C.WEIGHTS] = np.append(v[q * c:q * c + Lq - 1], 0.0)
                for t in (C.AGG, C.REP, C.FUT):
                    st[q, t] = np.zeros(Lq)
    elif call == "split":
        if taken:
            want = O.organize_gradients(v, C.M, C.P)[C.SPLIT_PART]
            assert np.array_equal(want.view(np.uint64), r.out.view(np.uint64)), case.id
    elif call == "update_gradient":
        if taken:
            parts = O.organize_gradients(v, C.M, C.P)
            for q in C.OWNED:
                O.fold(st[q, C.AGG], parts[q])
    elif call == "update_indirect":
        if rig.gbuf is None:
            rig.gbuf = np.zeros(O.gradient_buff_len(C.M, C.P))
        try:     # the buffer is overwritten before the overrun is noticed (MyIPFSClass.java:451)
            O.get_parameters_into(rig.gbuf, v.astype(">f8").tobytes())
            assert taken, case.id
        except IndexError:
            assert r.rc == RANGE, case.id
        if taken:
            O.fold(st[p, C.AGG], rig.gbuf)
    else:
        raise AssertionError(call)


def _run(O, rig, cases):
    bad = []
    for case in cases:
        r = rig.run(case)
        collected = rig.finish(case)
        got = rig.state()
        rig.prepare()
        if (r.rc, r.text) != CODES[case.id]:
            bad.append(f"{case.id}: returned {(r.rc, r.text)}, recorded {CODES[case.id]}")
            continue
        st = rig.model()
        _expect(O, rig, case, r, st, collected)
        for (q, t), want in st.items():
            if t != C.WEIGHTS:
                want = want + -0.0      # the probe
            if not np.array_equal(want.view(np.uint64), got[q, t].view(np.uint64)):
                bad.append(f"{case.id}: target {t} of partition {q} {'differs from the oracle' if r.rc >= 0 else 'changed'}")
    assert not bad, f"{len(bad)} of {len(cases)} cases:\n" + "\n".join(bad[:20])


@pytest.mark.parametrize("call", list(C.CALLS))
def test_source_kinds(O, rig, call):
    _run(O, rig, C.cases(call))


@pytest.mark.parametrize("L", C.SEAM_LENS)
def test_zero_copy_seam(O, ipls, L):
    """Pinned HOST_F64 / HOST_BE buckets of 8,191 and 8,192 values, 16 bytes
    and 8 bytes aligned, into a partition of L doubles: at L = 8192 the bucket
    is exactly the 65,536 bytes from which accumulate reads it in place (8-byte
    aligned is enough there, accumulate_async queues its own fold only from 16),
    at L = 8191 it is staged."""
    rig = C.Rig(ipls, torch, 0, 1, bucket_len=L)
    try:
        rig.prepare()
        bad = []
        for case in (c for c in C.seam_cases() if c.id.startswith(f"seam{L}.")):
            r = rig.run(case)
            rig.finish(case)
            got = rig.state()
            rig.prepare()
            if (r.rc, r.text) != CODES[case.id]:
                bad.append(f"{case.id}: returned {(r.rc, r.text)}, recorded {CODES[case.id]}")
                continue
            st = rig.model()
            if r.rc >= 0:
                O.fold(st[0, C.AGG], r.vals)
            for (q, t), want in st.items():
                if t != C.WEIGHTS:
                    want = want + -0.0
                if not np.array_equal(want.view(np.uint64), got[q, t].view(np.uint64)):
                    bad.append(f"{case.id}: target {t}")
        assert not bad, "\n".join(bad)
    finally:
        rig.close()
