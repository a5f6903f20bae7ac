#!/usr/bin/env python3
"""The float32 trainer boundary against what a trainer has without it, in one
process, at config C's geometry (16 partitions x 4,194,305 x 32 peers; 8.6 GB
of float buckets) and on a 64 Mi-value model:

 (a) widen first: every float bucket copied into a double bucket by torch
     (what ``bucket.double()`` does, into preallocated memory), then
     reduce_batch on the doubles -- both parts timed;
 (b) reduce_batch on the float buckets (k_reduce_narrow<FmtF32>); every partition's
     checksum must equal (a)'s before anything is reported;
 (c) UpdateGradient and GetPartitions at M = 64 Mi: ``.double()`` + DEV_F64 and
     DEV_F64 + ``.float()`` against the f32 kinds.

Timing is the README's: the span of K back-to-back launches between two HIP
events on the stream that runs them, divided by K; the median of REPS spans.
Fractions are of 8 TB/s over algorithmic bytes: (4K + 8) L P for (b),
(8K + 8) L P for the f64 fold.
Usage: f32_fold_probe.py [OUT.json] [REPS]
       f32_fold_probe.py --fold-only N    N launches of (b) and nothing else: the workload of a
                                          rocprofv3 --pmc pass (tools/pmc_traffic.py ... k_reduce_narrow)"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "ipls-java-api_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ipls  # noqa: E402

PEAK = 8e12
P, L, K = 16, 4194305, 32
M = 64 << 20
SPAN = 5


def span_ms(stream, fn, reps, span=SPAN):
    """Median over `reps` of (a span of `span` calls of fn between two events on `stream`) / span."""
    fn()
    stream.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(span):
            fn()
        e1.record(stream)
        stream.synchronize()
        out.append(e0.elapsed_time(e1) / span)
    return float(np.median(out)), [round(x, 4) for x in out]


def fold_only(n):
    s32 = (L + 3) // 4 * 4 + 64
    a32 = (torch.rand(P * K * s32, dtype=torch.float32, device="cuda") - 0.5) * 2e-2
    b32 = [[ipls.DeviceBuffer.from_tensor(a32[(q * K + k) * s32:(q * K + k) * s32 + L]) for k in range(K)]
           for q in range(P)]
    torch.cuda.synchronize()
    with ipls.Aggregator(n_partitions=P, bucket_len=L) as agg:
        for _ in range(n):
            agg.reduce_batch(0, b32)
        agg.sync()
        print(json.dumps({"launches": n, "launch": agg.last_launch(), "algorithmic_bytes": (4 * K + 8) * L * P,
                          "build": ipls.build_info()}))


def fold(reps):
    s32 = (L + 3) // 4 * 4 + 64          # floats per bucket slot: every bucket 16-B aligned
    s64 = (L + 1) // 2 * 2 + 32
    a32 = torch.empty(P * K * s32, dtype=torch.float32, device="cuda")
    a64 = torch.empty(P * K * s64, dtype=torch.float64, device="cuda")
    v32 = [a32[i * s32:i * s32 + L] for i in range(P * K)]
    v64 = [a64[i * s64:i * s64 + L] for i in range(P * K)]
    b32 = [[ipls.DeviceBuffer.from_tensor(v32[q * K + k]) for k in range(K)] for q in range(P)]
    b64 = [[ipls.DeviceBuffer.from_tensor(v64[q * K + k]) for k in range(K)] for q in range(P)]
    assert b32[0][0].kind == ipls.DEV_F32 and b64[0][0].kind == ipls.DEV_F64
    # the trainers' float buckets: the synthetic workload narrowed once (setup, not timed)
    for q in range(P):
        for k in range(K):
            ipls.synth_fill(b64[q][k], q, k, ipls.SEED)
    torch.cuda.synchronize()
    for i in range(P * K):
        v32[i].copy_(v64[i])
    a64.zero_()
    torch.cuda.synchronize()
    cur = torch.cuda.current_stream()

    def widen():
        for i in range(P * K):
            v64[i].copy_(v32[i])
    widen_ms, widen_all = span_ms(cur, widen, reps, span=1)
    torch.cuda.synchronize()
    res = {"P": P, "L": L, "K": K, "span": SPAN, "reps": reps}
    with ipls.Aggregator(n_partitions=P, bucket_len=L) as agg:
        st = torch.cuda.ExternalStream(agg.stream)
        f64_ms, f64_all = span_ms(st, lambda: agg.reduce_batch(0, b64), reps)
        li64 = agg.last_launch()
        sums64 = [agg.checksum(q) for q in range(P)]
        agg.reset()
        f32_ms, f32_all = span_ms(st, lambda: agg.reduce_batch(0, b32), reps)
        li32 = agg.last_launch()
        sums32 = [agg.checksum(q) for q in range(P)]
        assert li32["kernel"] == ipls.KERNEL_REDUCE_F32, li32
        assert sums32 == sums64, "the f32 fold and the widen-first fold differ"
        # interleaved once more, the other way round (order effects)
        f32_ms2, _ = span_ms(st, lambda: agg.reduce_batch(0, b32), reps)
        f64_ms2, _ = span_ms(st, lambda: agg.reduce_batch(0, b64), reps)
    b_f32, b_f64 = (4 * K + 8) * L * P, (8 * K + 8) * L * P
    res["a_widen_ms"] = round(widen_ms, 4)
    res["a_widen_spans_ms"] = widen_all
    res["a_fold_f64_ms"] = round(f64_ms, 4)
    res["a_fold_f64_ms_second_pass"] = round(f64_ms2, 4)
    res["a_fold_f64_spans_ms"] = f64_all
    res["a_fold_f64_frac_of_peak"] = round(b_f64 / (f64_ms * 1e-3) / PEAK, 4)
    res["a_fold_f64_launch"] = li64
    res["a_total_ms"] = round(widen_ms + f64_ms, 4)
    res["b_fold_f32_ms"] = round(f32_ms, 4)
    res["b_fold_f32_ms_second_pass"] = round(f32_ms2, 4)
    res["b_fold_f32_spans_ms"] = f32_all
    res["b_fold_f32_frac_of_peak"] = round(b_f32 / (f32_ms * 1e-3) / PEAK, 4)
    res["b_fold_f32_launch"] = li32
    res["b_algorithmic_bytes"] = b_f32
    res["checksums_equal"] = True
    res["b_over_a_fold"] = round(f32_ms / f64_ms, 4)
    res["b_over_a_total"] = round(f32_ms / (widen_ms + f64_ms), 4)
    del a32, a64, v32, v64
    torch.cuda.empty_cache()
    return res


def boundary(reps):
    Pm = 16
    g32 = (torch.rand(M, dtype=torch.float32, device="cuda") - 0.5) * 2e-2
    g64 = torch.empty(M, dtype=torch.float64, device="cuda")
    o64 = torch.empty(M, dtype=torch.float64, device="cuda")
    o32 = torch.empty(M, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    cur = torch.cuda.current_stream()
    auth = list(range(Pm))
    res = {"M": M, "P": Pm}
    with ipls.Aggregator(M, Pm) as a64, ipls.Aggregator(M, Pm) as a32:
        d32, d64 = ipls.DeviceBuffer.from_tensor(g32), ipls.DeviceBuffer.from_tensor(g64)
        s64, s32 = torch.cuda.ExternalStream(a64.stream), torch.cuda.ExternalStream(a32.stream)
        w_ms, _ = span_ms(cur, lambda: g64.copy_(g32), reps)
        a64.UpdateGradient(d64, auth)      # from here on AGG is read too (the steady state of a round)
        a32.UpdateGradient(d32, auth)
        u64_ms, _ = span_ms(s64, lambda: a64.UpdateGradient(d64, auth), reps)
        u32_ms, _ = span_ms(s32, lambda: a32.UpdateGradient(d32, auth), reps)
        assert [a32.checksum(p) for p in range(Pm)] == [a64.checksum(p) for p in range(Pm)]
        res["update_gradient"] = {"parent_widen_ms": round(w_ms, 4), "parent_dev_f64_ms": round(u64_ms, 4),
                                  "parent_total_ms": round(w_ms + u64_ms, 4), "f32_ms": round(u32_ms, 4),
                                  "f32_over_parent": round(u32_ms / (w_ms + u64_ms), 4)}
        for a in (a64, a32):
            a.AggregatePartition(ipls.ALL_PARTITIONS)
        b64, b32 = ipls.DeviceBuffer.from_tensor(o64), ipls.DeviceBuffer.from_tensor(o32)
        n_ms, _ = span_ms(cur, lambda: o32.copy_(o64), reps)
        p64_ms, _ = span_ms(s64, lambda: a64.GetPartitions(out=b64), reps)
        keep = o64.float()
        p32_ms, _ = span_ms(s32, lambda: a32.GetPartitions(out=b32), reps)
        torch.cuda.synchronize()
        assert torch.equal(keep.view(torch.int32), o32.view(torch.int32)), "GetPartitions f32 != f64 narrowed"
        res["get_partitions"] = {"parent_dev_f64_ms": round(p64_ms, 4), "parent_narrow_ms": round(n_ms, 4),
                                 "parent_total_ms": round(p64_ms + n_ms, 4), "f32_ms": round(p32_ms, 4),
                                 "f32_over_parent": round(p32_ms / (p64_ms + n_ms), 4)}
    return res


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--fold-only":
        fold_only(int(sys.argv[2]))
        sys.exit(0)
    out = sys.argv[1] if len(sys.argv) > 1 else None
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    result = {"device": torch.cuda.get_device_name(0), "fold": fold(reps), "boundary": boundary(reps)}
    text = json.dumps(result, indent=1)
    print(text)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(text + "\n")
