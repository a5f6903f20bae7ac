#!/usr/bin/env python3
"""The fused round over trainer-format buckets (k_round_narrow) against the
three steps it replaces, in one process on the same buckets, for f32, half and
bf16 buckets with averages of the same format, at three shapes:

  C    config C's 16 partitions x 4,194,305 x 32 peers
  one  one partition of 4,194,305 x 32 peers
  eth  ETHModel's 3 x 147,870 x 3

Per format and shape:
 (r) ``aggregate_round`` into a device buffer of the format -- with this
     library one fused launch (after the count pre-pass), with a library from
     before the fused kernel (``IPLS_AGG_LIB``, tools/build_rev_lib.sh) the
     three steps inside the call;
 (3) the three explicit calls: ``reduce_batch(ACCUM)``, ``AggregatePartition``
     of the range, ``GetPartitions(out=...)``;
 (f) ``reduce_batch`` alone (k_reduce_narrow), for the fold's share of peak in
     the same process;
 the checksum of W must be equal across (r) and (3), all partitions, and the
 averages bit for bit, before anything is reported.
A repeated round is repeatable work: AGG and REP are zero after every round.

Timing is the README's: the span of 5 back-to-back calls between two HIP events
on the handle's stream, divided by 5; the median of REPS spans, with the spread
(max - min of the REPS).  Fractions are of 8 TB/s over algorithmic bytes with
s the element size: (K s + 8 + s) L P for the fused round, (K s + 32 + s) L P
for the three steps, (K s + 8) L P for the fold.
Usage: narrow_round_probe.py [OUT.json] [REPS]
       narrow_round_probe.py --round-only N FMT   N rounds of (r) at config C and nothing else: the
                                                  workload of a counters-only rocprofv3 --pmc pass"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "ipls-java-api_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ipls  # noqa: E402

PEAK = 8e12
SPAN = 5
SHAPES = {"C": (16, 4194305, 32), "one": (1, 4194305, 32), "eth": (3, 147870, 3)}
TDT = {"f32": torch.float32, "half": torch.float16, "bf16": torch.bfloat16}
ESZ = {"f32": 4, "half": 2, "bf16": 2}
KERNELS = {1: "k_reduce", 2: "k_round", 5: "k_reduce_narrow (f32)", 6: "k_reduce_narrow (16-bit)",
           7: "k_round_narrow (f32)", 8: "k_round_narrow (16-bit)"}


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


def arena(fmt):
    """Config C's buckets of the format, every one 16-B aligned, 1.0 in the
    count slot of each shape's length; the smaller shapes use the first ones."""
    P, L, K = SHAPES["C"]
    per16 = 16 // ESZ[fmt]
    slot = (L + per16 - 1) // per16 * per16 + 64
    a = torch.empty(P * K * slot, dtype=TDT[fmt], device="cuda")
    step = 32 * slot                                      # 32 buckets at a time: bounded temporaries
    for lo in range(0, a.numel(), step):
        n = min(step, a.numel() - lo)
        a[lo:lo + n] = ((torch.rand(n, dtype=torch.float32, device="cuda") - 0.5) * 2e-2).to(TDT[fmt])
    torch.cuda.synchronize()
    return a, slot


def table(a, slot, shape):
    P, L, K = SHAPES[shape]
    v = [a[i * slot:i * slot + L] for i in range(P * K)]
    for t in v:
        t[L - 1] = 1.0
    torch.cuda.synchronize()
    return [[ipls.DeviceBuffer.from_tensor(v[q * K + k]) for k in range(K)] for q in range(P)]


def round_only(n, fmt):
    P, L, K = SHAPES["C"]
    a, slot = arena(fmt)
    b = table(a, slot, "C")
    out = torch.empty(P * (L - 1) + 8, dtype=TDT[fmt], device="cuda")
    ob = ipls.DeviceBuffer.from_tensor(out[:P * (L - 1)])
    torch.cuda.synchronize()
    with ipls.Aggregator(n_partitions=P, bucket_len=L) as agg:
        for _ in range(n):
            agg.aggregate_round(0, b, out=ob)
        agg.sync()
        s = ESZ[fmt]
        print(json.dumps({"rounds": n, "fmt": fmt, "launch": agg.last_launch(),
                          "algorithmic_bytes": (K * s + 8 + s) * L * P, "algorithmic_write_bytes": (8 + s) * L * P,
                          "build": ipls.build_info()}))


def probe(reps):
    res = {"span": SPAN, "reps": reps, "shapes": {k: dict(zip("PLK", v)) for k, v in SHAPES.items()}}
    for fmt in ("f32", "half", "bf16"):
        s = ESZ[fmt]
        a, slot = arena(fmt)
        res[fmt] = {}
        for shape in ("C", "one", "eth"):                 # eth last: its count slots overwrite values of the others
            P, L, K = SHAPES[shape]
            b = table(a, slot, shape)
            n = P * (L - 1)
            o_r = torch.zeros(n + 8, dtype=TDT[fmt], device="cuda")
            o_3 = torch.zeros(n + 8, dtype=TDT[fmt], device="cuda")
            b_r, b_3 = ipls.DeviceBuffer.from_tensor(o_r[:n]), ipls.DeviceBuffer.from_tensor(o_3[:n])
            torch.cuda.synchronize()
            with ipls.Aggregator(n_partitions=P, bucket_len=L) as agg:
                st = torch.cuda.ExternalStream(agg.stream)

                def three():
                    agg.reduce_batch(0, b, start_mode=ipls.START_ACCUM)
                    agg.AggregatePartition(ipls.ALL_PARTITIONS)
                    agg.GetPartitions(out=b_3)

                def fused():
                    agg.aggregate_round(0, b, out=b_r)

                r_ms, r_sp, r_all = span_ms(st, fused, reps)
                li = agg.last_launch()
                sums_r = [agg.checksum(q, ipls.TGT_WEIGHTS) for q in range(P)]
                t_ms, t_sp, t_all = span_ms(st, three, reps)
                sums_3 = [agg.checksum(q, ipls.TGT_WEIGHTS) for q in range(P)]
                assert sums_r == sums_3, f"{fmt} {shape}: W differs between the round and the three steps"
                agg.sync()
                assert torch.equal(o_r.view(torch.uint8), o_3.view(torch.uint8)), f"{fmt} {shape}: averages differ"
                f_ms, f_sp, f_all = span_ms(st, lambda: agg.reduce_batch(0, b), reps)
                fli = agg.last_launch()
                agg.reset()
                r2_ms, r2_sp, _ = span_ms(st, fused, reps)   # once more, after the others (order effects)
            by_r, by_3, by_f = (K * s + 8 + s) * L * P, (K * s + 32 + s) * L * P, (K * s + 8) * L * P
            res[fmt][shape] = {
                "round_ms": round(r_ms, 4), "round_ms_second_pass": round(r2_ms, 4), "round_spans_ms": r_all,
                "round_spread_ms": round(r_sp, 4), "round_kernel": KERNELS.get(li["kernel"], li["kernel"]),
                "round_launch": li, "round_algorithmic_bytes": by_r,
                "round_frac_of_peak": round(by_r / (r_ms * 1e-3) / PEAK, 4),
                "three_steps_ms": round(t_ms, 4), "three_steps_spans_ms": t_all, "three_steps_spread_ms": round(t_sp, 4),
                "three_steps_algorithmic_bytes": by_3,
                "fold_ms": round(f_ms, 4), "fold_spans_ms": f_all, "fold_spread_ms": round(f_sp, 4),
                "fold_kernel": KERNELS.get(fli["kernel"], fli["kernel"]),
                "fold_frac_of_peak": round(by_f / (f_ms * 1e-3) / PEAK, 4),
                "round_over_three_steps": round(r_ms / t_ms, 4),
                "bytes_round_over_three_steps": round(by_r / by_3, 4),
                "checksums_equal": True, "averages_equal": True,
            }
            print(fmt, shape, json.dumps(res[fmt][shape]), flush=True)
            del o_r, o_3, b
        del a
        torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--round-only":
        round_only(int(sys.argv[2]), sys.argv[3])
        sys.exit(0)
    out = sys.argv[1] if len(sys.argv) > 1 else None
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    result = {"device": torch.cuda.get_device_name(0), "build": ipls.build_info(), "probe": probe(reps)}
    text = json.dumps(result, indent=1)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(text + "\n")
    else:
        print(text)
