#!/usr/bin/env python3
"""The half-precision trainer boundary against what a trainer has without it,
in one process, at config C's geometry (16 partitions x 4,194,305 x 32 peers;
4.3 GB of 16-bit buckets) and on a 64 Mi-value model, for each of the two
formats (IEEE binary16 "half", bfloat16 "bf16"):

 (h) reduce_batch on the 16-bit buckets (k_reduce_narrow<FmtF16 | FmtBF16>);
 (f) reduce_batch on the same values widened to float (exact): k_reduce_narrow<FmtF32>;
 (w) torch ``.float()`` of every bucket (into preallocated memory), then (f) --
     the only route a user had: both parts timed;
 (d) reduce_batch on the same values as doubles: the f64 fold;
 every partition's checksum must be equal across the four before anything is
 reported;
 (c) UpdateGradient and GetPartitions at M = 64 Mi: ``.float()`` + DEV_F32 and
     DEV_F32 + ``.to(fmt)`` against the 16-bit kinds.

Timing is the README's: the span of 5 back-to-back launches between two HIP
events on the stream that runs them, divided by 5; the median of REPS spans,
with the spread (max - min of the REPS) beside it.  Fractions are of 8 TB/s
over algorithmic bytes: (2K + 8) L P for (h), (4K + 8) L P for (f),
(8K + 8) L P for (d).
Usage: h16_fold_probe.py [OUT.json] [REPS]
       h16_fold_probe.py --fold-only N FMT   N launches of (h) and nothing else: the workload of a
                                             counters-only rocprofv3 --pmc pass"""
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
TDT = {"half": torch.float16, "bf16": torch.bfloat16}


def span_ms(stream, fn, reps, span=SPAN):
    """(median, spread, all) over `reps` of (a span of `span` calls of fn between two events on `stream`) / span."""
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
    return float(np.median(out)), float(max(out) - min(out)), [round(x, 4) for x in out]


def fold_only(n, fmt):
    s16 = (L + 7) // 8 * 8 + 64
    a16 = ((torch.rand(P * K * s16, dtype=torch.float32, device="cuda") - 0.5) * 2e-2).to(TDT[fmt])
    b16 = [[ipls.DeviceBuffer.from_tensor(a16[(q * K + k) * s16:(q * K + k) * s16 + L]) for k in range(K)]
           for q in range(P)]
    torch.cuda.synchronize()
    with ipls.Aggregator(n_partitions=P, bucket_len=L) as agg:
        for _ in range(n):
            agg.reduce_batch(0, b16)
        agg.sync()
        print(json.dumps({"launches": n, "fmt": fmt, "launch": agg.last_launch(),
                          "algorithmic_bytes": (2 * K + 8) * L * P, "build": ipls.build_info()}))


def fold(reps):
    s16 = (L + 7) // 8 * 8 + 64          # elements per bucket slot: every bucket 16-B aligned
    s32 = (L + 3) // 4 * 4 + 64
    s64 = (L + 1) // 2 * 2 + 32
    a32 = torch.empty(P * K * s32, dtype=torch.float32, device="cuda")
    a64 = torch.empty(P * K * s64, dtype=torch.float64, device="cuda")
    v32 = [a32[i * s32:i * s32 + L] for i in range(P * K)]
    v64 = [a64[i * s64:i * s64 + L] for i in range(P * K)]
    b32 = [[ipls.DeviceBuffer.from_tensor(v32[q * K + k]) for k in range(K)] for q in range(P)]
    b64 = [[ipls.DeviceBuffer.from_tensor(v64[q * K + k]) for k in range(K)] for q in range(P)]
    cur = torch.cuda.current_stream()
    res = {"P": P, "L": L, "K": K, "span": SPAN, "reps": reps}
    b_h16, b_f32, b_f64 = (2 * K + 8) * L * P, (4 * K + 8) * L * P, (8 * K + 8) * L * P
    for fmt in ("half", "bf16"):
        a16 = torch.empty(P * K * s16, dtype=TDT[fmt], device="cuda")
        v16 = [a16[i * s16:i * s16 + L] for i in range(P * K)]
        b16 = [[ipls.DeviceBuffer.from_tensor(v16[q * K + k]) for k in range(K)] for q in range(P)]
        assert b16[0][0].dtype == fmt
        # the trainers' 16-bit buckets: the synthetic workload narrowed (setup, not timed),
        # then the very same values as floats and as doubles (both widenings exact)
        for q in range(P):
            for k in range(K):
                ipls.synth_fill(b64[q][k], q, k, ipls.SEED)
        torch.cuda.synchronize()
        for i in range(P * K):
            v16[i].copy_(v64[i])
        for i in range(P * K):
            v64[i].copy_(v16[i])
        a32.zero_()
        torch.cuda.synchronize()

        def widen():
            for i in range(P * K):
                v32[i].copy_(v16[i])
        w_ms, w_spread, w_all = span_ms(cur, widen, reps, span=1)
        torch.cuda.synchronize()
        with ipls.Aggregator(n_partitions=P, bucket_len=L) as agg:
            st = torch.cuda.ExternalStream(agg.stream)
            h_ms, h_spread, h_all = span_ms(st, lambda: agg.reduce_batch(0, b16), reps)
            li = agg.last_launch()
            assert li["kernel"] == ipls.KERNEL_REDUCE_H16 and li["seqf"] == 1, li
            sums_h = [agg.checksum(q) for q in range(P)]
            agg.reset()
            f_ms, f_spread, f_all = span_ms(st, lambda: agg.reduce_batch(0, b32), reps)
            assert agg.last_launch()["kernel"] == ipls.KERNEL_REDUCE_F32
            sums_f = [agg.checksum(q) for q in range(P)]
            agg.reset()
            d_ms, d_spread, d_all = span_ms(st, lambda: agg.reduce_batch(0, b64), reps)
            sums_d = [agg.checksum(q) for q in range(P)]
            agg.reset()
            # (w) as one sequence: the widening pass, then the f32 fold of its output
            widen()
            torch.cuda.synchronize()
            agg.reduce_batch(0, b32)
            sums_w = [agg.checksum(q) for q in range(P)]
            assert sums_h == sums_f == sums_d == sums_w, f"{fmt}: the four folds differ"
            # once more the other way round (order effects)
            h_ms2, _, _ = span_ms(st, lambda: agg.reduce_batch(0, b16), reps)
        spread = max(h_spread, w_spread + f_spread)
        res[fmt] = {
            "h16_fold_ms": round(h_ms, 4), "h16_fold_ms_second_pass": round(h_ms2, 4), "h16_fold_spans_ms": h_all,
            "h16_fold_spread_ms": round(h_spread, 4), "h16_fold_frac_of_peak": round(b_h16 / (h_ms * 1e-3) / PEAK, 4),
            "h16_launch": li, "h16_algorithmic_bytes": b_h16,
            "f32_fold_ms": round(f_ms, 4), "f32_fold_spans_ms": f_all, "f32_fold_spread_ms": round(f_spread, 4),
            "f32_fold_frac_of_peak": round(b_f32 / (f_ms * 1e-3) / PEAK, 4),
            "float_pass_ms": round(w_ms, 4), "float_pass_spans_ms": w_all, "float_pass_spread_ms": round(w_spread, 4),
            "float_then_f32_fold_ms": round(w_ms + f_ms, 4),
            "f64_fold_ms": round(d_ms, 4), "f64_fold_spans_ms": d_all, "f64_fold_spread_ms": round(d_spread, 4),
            "f64_fold_frac_of_peak": round(b_f64 / (d_ms * 1e-3) / PEAK, 4),
            "checksums_equal": True,
            "h16_over_f32_fold": round(h_ms / f_ms, 4),
            "h16_over_float_then_f32_fold": round(h_ms / (w_ms + f_ms), 4),
            "probe_spread_ms": round(spread, 4),
            "h16_beats_float_then_f32_by_more_than_spread": bool((w_ms + f_ms) - h_ms > spread),
        }
        print(fmt, json.dumps(res[fmt]), flush=True)
        del a16, v16, b16
        torch.cuda.empty_cache()
    del a32, a64, v32, v64
    torch.cuda.empty_cache()
    return res


def boundary(reps):
    Pm = 16
    res = {"M": M, "P": Pm}
    cur = torch.cuda.current_stream()
    auth = list(range(Pm))
    for fmt in ("half", "bf16"):
        g16 = ((torch.rand(M, dtype=torch.float32, device="cuda") - 0.5) * 2e-2).to(TDT[fmt])
        g32 = torch.empty(M, dtype=torch.float32, device="cuda")
        o32 = torch.empty(M, dtype=torch.float32, device="cuda")
        o16 = torch.empty(M, dtype=TDT[fmt], device="cuda")
        n16 = torch.empty(M, dtype=TDT[fmt], device="cuda")
        torch.cuda.synchronize()
        with ipls.Aggregator(M, Pm) as a32, ipls.Aggregator(M, Pm) as a16:
            d16, d32 = ipls.DeviceBuffer.from_tensor(g16), ipls.DeviceBuffer.from_tensor(g32)
            s32, s16 = torch.cuda.ExternalStream(a32.stream), torch.cuda.ExternalStream(a16.stream)
            w_ms, w_sp, _ = span_ms(cur, lambda: g32.copy_(g16), reps)
            a32.UpdateGradient(d32, auth)      # from here on AGG is read too (the steady state of a round)
            a16.UpdateGradient(d16, auth)
            u32_ms, u32_sp, _ = span_ms(s32, lambda: a32.UpdateGradient(d32, auth), reps)
            u16_ms, u16_sp, _ = span_ms(s16, lambda: a16.UpdateGradient(d16, auth), reps)
            assert [a16.checksum(p) for p in range(Pm)] == [a32.checksum(p) for p in range(Pm)]
            res[fmt] = {"update_gradient": {
                "float_pass_ms": round(w_ms, 4), "dev_f32_ms": round(u32_ms, 4),
                "float_then_f32_ms": round(w_ms + u32_ms, 4), "h16_ms": round(u16_ms, 4),
                "spread_ms": round(max(u16_sp, w_sp + u32_sp), 4),
                "h16_over_float_then_f32": round(u16_ms / (w_ms + u32_ms), 4)}}
            for a in (a32, a16):
                a.AggregatePartition(ipls.ALL_PARTITIONS)
            b32, b16 = ipls.DeviceBuffer.from_tensor(o32), ipls.DeviceBuffer.from_tensor(o16)
            p32_ms, p32_sp, _ = span_ms(s32, lambda: a32.GetPartitions(out=b32), reps)
            n_ms, n_sp, _ = span_ms(cur, lambda: n16.copy_(o32), reps)
            p16_ms, p16_sp, _ = span_ms(s16, lambda: a16.GetPartitions(out=b16), reps)
            torch.cuda.synchronize()
            assert torch.equal(n16.view(torch.int16), o16.view(torch.int16)), "GetPartitions 16-bit != f32 narrowed"
            res[fmt]["get_partitions"] = {
                "dev_f32_ms": round(p32_ms, 4), "narrow_pass_ms": round(n_ms, 4),
                "f32_then_narrow_ms": round(p32_ms + n_ms, 4), "h16_ms": round(p16_ms, 4),
                "spread_ms": round(max(p16_sp, p32_sp + n_sp), 4),
                "h16_over_f32_then_narrow": round(p16_ms / (p32_ms + n_ms), 4)}
        del g16, g32, o32, o16, n16
        torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--fold-only":
        fold_only(int(sys.argv[2]), sys.argv[3])
        sys.exit(0)
    out = sys.argv[1] if len(sys.argv) > 1 else None
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    result = {"device": torch.cuda.get_device_name(0), "fold": fold(reps), "boundary": boundary(reps)}
    text = json.dumps(result, indent=1)
    print(text)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(text + "\n")
