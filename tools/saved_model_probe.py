#!/usr/bin/env python3
"""Rates of the saved-model path: the device kernels through
tools/saved_model_sweep.hip (pack, boxed pack, apply against the aligned
k_bswap64 yardstick, K launches between two HIP events, min and max of five
repeats), then save_model end to end into host memory against the way to the
same bytes without it: one ipls_agg_read(..., HOST_BE) per partition plus the
framing on the host.  Config C geometry, 16 x 4,194,304, every partition in
the map.  Writes one JSON document.

    make -C ipls-java-api_amd sweeps                     # where the compiler is
    python tools/saved_model_probe.py --out profiles/saved_model_probe.json
"""
import argparse
import ctypes
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "ipls-java-api_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--partitions", type=int, default=16)
    ap.add_argument("--bucket-len", type=int, default=4194304)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    P, L = a.partitions, a.bucket_len
    sweep = ROOT / "ipls-java-api_amd" / "lib" / "saved_model_sweep"
    if not sweep.exists():
        sys.exit(f"{sweep} not built: make -C ipls-java-api_amd sweeps")
    r = subprocess.run([str(sweep), str(P), str(L), str(a.launches), str(a.reps)], capture_output=True, text=True,
                       timeout=600, check=True)
    res = {"device": json.loads(r.stdout.strip().splitlines()[-1])}

    import numpy as np
    import torch  # noqa: F401 -- before the library (ipls._native.lib)
    import ipls
    from ipls import _native as N
    lib = N.lib()
    with ipls.Aggregator(n_partitions=P, bucket_len=L) as agg:
        rng = np.random.default_rng(1)
        for p in range(P):
            agg.cache_partition(p, rng.standard_normal(L))
        parts = (ctypes.c_int32 * P)(*range(P))
        total = lib.ipls_agg_save_model(agg.handle, parts, P, N.TGT_WEIGHTS, None, 0)
        out = np.empty(total, dtype=np.uint8)
        bufs = [np.empty(8 * L, dtype=np.uint8) for _ in range(P)]
        ptrs = (ctypes.c_void_p * P)(*[b.ctypes.data for b in bufs])
        lens = (ctypes.c_int64 * P)(*[L] * P)
        ref = np.empty(total, dtype=np.uint8)

        def save():
            assert lib.ipls_agg_save_model(agg.handle, parts, P, N.TGT_WEIGHTS, out.ctypes.data, total) == total

        def read_loop():
            for p in range(P):
                assert lib.ipls_agg_read(agg.handle, p, N.TGT_WEIGHTS, bufs[p].ctypes.data, L, N.HOST_BE) == 0
            assert lib.ipls_saved_encode(parts, P, ptrs, lens, N.HOST_BE, ref.ctypes.data, total) == total

        times = {"save_model": [], "read_loop_plus_host_framing": []}
        for fn in (save, read_loop):
            fn()                                             # warm-up: staging, pinned slots
        assert np.array_equal(out, ref), "the two ways give different bytes"
        for _ in range(a.reps):
            for name, fn in (("save_model", save), ("read_loop_plus_host_framing", read_loop)):
                t0 = time.perf_counter()
                fn()
                times[name].append(time.perf_counter() - t0)
        res["end_to_end"] = {"file_bytes": int(total)}
        for name, ts in times.items():
            res["end_to_end"][name + "_ms"] = [round(1e3 * min(ts), 2), round(1e3 * max(ts), 2)]
            res["end_to_end"][name + "_gbs"] = [round(total / max(ts) / 1e9, 2), round(total / min(ts) / 1e9, 2)]
    res["build"] = N.build_info()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
