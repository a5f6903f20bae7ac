#!/usr/bin/env python3
"""The per-arrival fold of one trainer-format bucket: ``ipls_agg_accumulate`` of
one DEV f32 bucket and one DEV bf16 bucket into a non-zero accumulator (ACCUM),
at three partition lengths:

  eth  147,870     (ETHModel's partition)
  1M   1,048,576
  4M   4,194,304

One process measures one library: this tree's (k_fold1_narrow, pointers as
kernel arguments) or, with ``IPLS_AGG_LIB`` naming a build of an earlier
revision (tools/build_rev_lib.sh), that one (k_reduce_narrow with K = 1 behind a
table upload).  Run the two in alternating processes on one box and compare the
medians; two runs of the same build give the spread a difference has to exceed.
Both go through the ctypes binding, so the host side of a call is the same.

Timing is the README's: the span of SPAN back-to-back calls between two HIP
events on the handle's stream, divided by SPAN; the median of REPS spans and
their spread (max - min).  Fractions are of 8 TB/s over the algorithmic
(s + 16) L bytes: 20 B per element for floats, 18 B for bfloat16.
Usage: narrow_fold1_probe.py [OUT.json] [REPS]
       narrow_fold1_probe.py --launch-only N FMT   N folds at 4M and nothing else: the workload of a
                                                   counters-only rocprofv3 --pmc pass"""
import ctypes
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "ipls-java-api_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ipls  # noqa: E402
from ipls import _native as _N  # noqa: E402

if os.environ.get("IPLS_AGG_LIB"):
    # a build of an earlier revision lacks the entry points added since: bind what it has
    _L = ctypes.CDLL(os.environ["IPLS_AGG_LIB"])
    for _name in [n for n in _N.SIGNATURES if not hasattr(_L, n)]:
        del _N.SIGNATURES[_name]

PEAK = 8e12
SPAN = 20
SIZES = {"eth": 147870, "1M": 1048576, "4M": 4194304}
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
ESZ = {"f32": 4, "bf16": 2}
KERNELS = {3: "k_fold1", 5: "k_reduce_narrow (f32)", 6: "k_reduce_narrow (16-bit)", 9: "k_fold1_narrow (f32)",
           10: "k_fold1_narrow (16-bit)"}


def span_ms(stream, fn, reps, span=SPAN):
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
    return float(np.median(out)), float(max(out) - min(out)), [round(x, 5) for x in out]


def bucket(fmt, L):
    torch.manual_seed(L)          # the same values in every process: checksums compare across builds
    t = ((torch.rand(L + 8, dtype=torch.float32, device="cuda") - 0.5) * 2e-2).to(TDT[fmt])
    t[L - 1] = 1.0
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t, ipls.DeviceBuffer.from_tensor(t[:L])


def handle(L):
    agg = ipls.Aggregator(n_partitions=1, bucket_len=L)
    agg.Update(np.full(L, 0.5), 0)          # a live accumulator: every timed fold is ACCUM
    return agg


def launch_only(n, fmt):
    L = SIZES["4M"]
    keep, d = bucket(fmt, L)
    with handle(L) as agg:
        for _ in range(n):
            agg._chk(agg._lib.ipls_agg_accumulate(agg._h, 0, ipls.TGT_AGG, d.ptr, d.n, d.kind))
        agg.sync()
        print(json.dumps({"folds": n, "fmt": fmt, "L": L, "launch": agg.last_launch(),
                          "algorithmic_write_bytes": 8 * L, "build": ipls.build_info()}))


def probe(reps):
    res = {"span": SPAN, "reps": reps, "sizes": SIZES}
    for fmt in ("f32", "bf16"):
        res[fmt] = {}
        for name, L in SIZES.items():
            keep, d = bucket(fmt, L)
            with handle(L) as agg:
                st = torch.cuda.ExternalStream(agg.stream)
                lib, h = agg._lib, agg._h

                def fold():
                    rc = lib.ipls_agg_accumulate(h, 0, ipls.TGT_AGG, d.ptr, d.n, d.kind)
                    if rc < 0:
                        agg._chk(rc)
                ms, sp, allv = span_ms(st, fold, reps)
                li = agg.last_launch()
                ms2, sp2, _ = span_ms(st, fold, reps)      # once more (order effects)
                csum = agg.checksum(0, ipls.TGT_AGG)
            by = (ESZ[fmt] + 16) * L
            res[fmt][name] = {"L": L, "ms": round(ms, 5), "ms_second_pass": round(ms2, 5), "spans_ms": allv,
                              "spread_ms": round(sp, 5), "kernel": KERNELS.get(li["kernel"], li["kernel"]),
                              "launch": li, "algorithmic_bytes": by,
                              "frac_of_peak": round(by / (ms * 1e-3) / PEAK, 4), "checksum": csum}
            print(fmt, name, json.dumps(res[fmt][name]), flush=True)
            del keep
    return res


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--launch-only":
        launch_only(int(sys.argv[2]), sys.argv[3])
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
