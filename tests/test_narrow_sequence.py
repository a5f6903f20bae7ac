"""The committed plans of tests/test_gpu_stateful_narrow.py can see the
mistakes they are for -- shown on the oracle alone, no GPU.

Coverage: every op class of the vocabulary occurs in each plan, and so does
every situation in which a flag mistake changes the bits (a narrow arrival into
a flagged accumulator over stale sums, a fused round with REP flagged over
stale sums, a save of a flagged accumulator, ...).  The scripted prefix of
narrow_sequence.plan sets these situations up, so every seed satisfies every
condition; the random steps after it meet them again in other orders (seeds
1, 2, 3, 5, 6, 8 at the short geometry and 7 at the tile geometry are the
ones whose random steps alone also expose all nine mistakes: 4 does not reach
a SET into a flagged accumulator that a later read shows).

Sensitivity: each plan is replayed through nine deliberately wrong variants of
the model (narrow_sequence.BUGS); each must differ from the true model at a
value the GPU test compares.
"""
import numpy as np
import pytest

import narrow_fmt as F
import narrow_sequence as S
import saved_model_writer as W

# the (seed, geometry, steps) of every case tests/test_gpu_stateful_narrow.py commits
PLANS = sorted({(seed, geom, steps) for seed, geom, steps, _, _, _ in S.CASES})

OP_CLASSES = {o for o, _ in S.OPS}
CONDITIONS = (
    [("arrival", form, where) for form in ("dev", "devoff", "host", "pinned") for where in ("stale", "nonzero")]
    + ["batch_accum_mixed", ("batch", "zero"), ("batch", "accum"), ("batch", "first"),
       "round_narrow", "round_rep_nonzero", "round_rep_flagged_stale", "round_agg_nonzero",
       ("round_fallback", "misalign"), ("round_fallback", "narrow_to_f64"), ("round_fallback", "f64_to_narrow"),
       "queue_mixed_witness", "save_flagged_stale", ("load_then_accum", "set"), ("load_then_accum", "blend"),
       ("init_narrow", "all_nonzero"), ("init_dlist", "all_nonzero"), "chunked_stopped"]
    + [("refuse", w) for w in ("cache", "areplica", "leaving", "other", "mixed")])

_RUNS = {}


def _run(seed, geom, steps, bugs=(), with_prefix=True):
    """(outputs of every step + the final state, events) of one replay; the true model's replay is shared."""
    key = (seed, geom, steps, tuple(bugs), with_prefix)
    if key not in _RUNS:
        lengths, offsets = S.geometry(*S.GEOMETRIES[geom])
        pool = S.Pool(seed, lengths, offsets)
        m = S.Model(pool, bugs=bugs)
        outs = [m.apply(s) for s in S.plan(seed, lengths, offsets, steps, with_prefix=with_prefix)]
        outs.append(m.final())
        _RUNS[key] = (outs, m.events)
    return _RUNS[key]


def test_geometries():
    lengths, offsets = S.geometry(*S.GEOMETRIES["short"])
    assert lengths == [5004, 5004, 5004, 5001] and [o % 16 for o in offsets] == [0, 11, 6, 1]
    lengths, offsets = S.geometry(*S.GEOMETRIES["tile"])
    T, b = S.TILE16, S.BLOCK16
    assert T <= 32768 and offsets[1] % 2 == 1                      # an odd chunk
    for L in lengths:                                              # one full tile, vector steps of 4 per lane, a remainder
        assert L // T == 1 and (L % T) >= 4 * b and (L % T) % 4 != 0


def test_pool_buckets():
    lengths, offsets = S.geometry(*S.GEOMETRIES["short"])
    pool = S.Pool(1, lengths, offsets)
    assert 10 <= len(pool.f64) <= 12 and all(10 <= len(pool.bits[f]) <= 12 for f in S.NARROW)
    for fmt in S.NARROW:
        for k, w in enumerate(pool.wide[fmt][:S.N_GENERAL[fmt]]):
            assert np.all(np.isfinite(w)) and all(w[L - 1] == 1.0 for L in lengths)
            if k != 1:                                              # bucket 1 is bucket 0 negated: its zeros are +0.0
                assert np.count_nonzero(np.signbit(w) & (w == 0)) >= 20, "-0.0 in many positions"
            assert np.any((w != 0) & (np.abs(w) < np.finfo(np.float32).tiny if fmt != "half" else np.abs(w) < 2.0 ** -14)), "subnormals"
            big = {"f32": float(np.finfo(np.float32).max), "half": 65504.0, "bf16": float(F.widen(np.array([0x7F7F], np.uint16), "bf16")[0])}
            assert np.any(np.abs(w) == big[fmt]), "the largest finite value"
        s = pool.wide[fmt][0] + pool.wide[fmt][1]                  # the cancelling pair
        assert np.count_nonzero(s) == len({L - 1 for L in lengths})
        # the order witness: a reorder across formats changes the bits
        a, one, c = pool.f64[S.WPOS[fmt]], pool.wide[fmt][S.ONES], pool.f64[S.WNEG[fmt]]
        assert np.all(((0.0 + a) + one) + c == 0.0) and np.all(((0.0 + a) + c) + one == 1.0)
    for k, g in enumerate(pool.f64[:8]):
        assert k == 1 or np.count_nonzero(np.signbit(g) & (g == 0)) >= 20
        assert np.any(np.abs(g) == 5e-324) and np.all(np.isfinite(g)) and all(g[L - 1] == 1.0 for L in lengths)


@pytest.mark.parametrize("seed,geom,steps", PLANS)
def test_plan_coverage(seed, geom, steps):
    outs, events = _run(seed, geom, steps)
    missing = [o for o in sorted(OP_CLASSES) if o not in events] + [c for c in CONDITIONS if c not in events]
    assert not missing, f"seed {seed} {geom}: the plan never reaches {missing}"
    # the same plan from the same seed: every draw is made up front
    lengths, offsets = S.geometry(*S.GEOMETRIES[geom])
    assert S.plan(seed, lengths, offsets, steps) == S.plan(seed, lengths, offsets, steps)


@pytest.mark.parametrize("with_prefix", (True, False), ids=("whole-plan", "random-steps-alone"))
@pytest.mark.parametrize("bug", sorted(S.BUGS))
@pytest.mark.parametrize("seed,geom,steps", PLANS)
def test_plan_sensitivity(seed, geom, steps, bug, with_prefix):
    """Each wrong variant of the model differs from the true one at a compared
    value -- of the whole plan, and of its random steps taken alone (the seeds
    are picked so that the latter holds too: the prefix is not what carries
    the test)."""
    true, _ = _run(seed, geom, steps, (), with_prefix)
    wrong, _ = _run(seed, geom, steps, (bug,), with_prefix)
    first = next((i for i, (a, b) in enumerate(zip(true, wrong)) if not S.same(a, b)), None)
    assert first is not None, f"seed {seed} {geom}: a library in which {S.BUGS[bug]} would pass"


def test_file_kinds_are_the_writer():
    """What the model returns for a save step is what saved_model_writer turns into bytes."""
    lengths, offsets = S.geometry(*S.GEOMETRIES["short"])
    pool = S.Pool(3, lengths, offsets)
    m = S.Model(pool)
    m.apply(dict(op="update64", p=1, tgt="agg", fmt="f64", k=2, form="host", off=0))
    (_, kind, (arrays, order)), = m.apply(dict(op="save_model", p=0, tgt="agg", auth=[1, 0], chunk_bytes=64))
    assert kind == "map" and order == [1, 0]
    assert W.write_map(arrays, order) == W.write_map({0: np.zeros(5004), 1: 0.0 + pool.f64[2][:5004]}, [1, 0])
