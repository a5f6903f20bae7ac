#!/usr/bin/env python3
"""SendGradients on the device against the routes it replaces, in one process.

    python tools/send_probe.py [--reps 10] [--parts 16] [--len 4194305] [--out profiles/send_flat/probe.json]

On `parts` partitions of `len` doubles (the count slot among them) it
interleaves, rep by rep:

  flat_f64 / flat_f32 / flat_bf16   ipls_agg_send_gradients from a DEV_F64 / DEV_F32 / DEV_BF16 vector into
                                    device texts (k_b64url_encode_flat; element loads for every format)
  frames                            ipls_agg_publish_partials of the same geometry into the same buffer
                                    (k_b64url_encode_frames: the same text bytes from aligned doubles)
  three_step                        today's route, per partition: ipls_agg_split to host doubles, the host
                                    frame (ipls_frame_encode), base64 on the CPU

Device legs are timed with HIP events on the handle's stream around one call
(table upload and launch included) after a warm-up of every leg; the host leg
with a host clock (it ends in a copy back).  Every leg's texts are compared
with the three-step route's once, before timing.  Prints and writes one JSON
object: per leg the times of every rep in ms, min / median / max, and GB/s of
algorithmic bytes (s + 32/3 per value for the flat legs, 8 + 32/3 for frames).
"""
import argparse
import base64
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "ipls-java-api_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parts", type=int, default=16)
    ap.add_argument("--len", type=int, default=4194305)
    ap.add_argument("--host-reps", type=int, default=3, help="reps that include the three-step host route")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "send_flat" / "probe.json"))
    a = ap.parse_args()
    import torch

    import ipls
    if not torch.cuda.is_available():
        sys.exit("send_probe: no GPU (a timing needs one)")
    P, L = a.parts, a.len
    n = P * (L - 1)
    agg = ipls.Aggregator(n_partitions=P, bucket_len=L)
    stream = torch.cuda.ExternalStream(agg.stream)
    g = torch.Generator(device="cuda").manual_seed(20261021)
    v32 = torch.randn(n, generator=g, device="cuda", dtype=torch.float32)
    src = {"flat_f64": v32.double(), "flat_f32": v32, "flat_bf16": v32.bfloat16()}
    esize = {"flat_f64": 8, "flat_f32": 4, "flat_bf16": 2}
    parts = list(range(P))
    origin = b"Qm" + b"x" * 44
    for p in parts:     # the publish leg reads W: give it real doubles
        agg.cache_partition(p, np.random.default_rng(p).standard_normal(L))
    text = (14 + 8 * L + len(origin) + 2) // 3 * 4                     # chars of one text; each starts on a 64-B boundary
    out = torch.empty(P * ((text + 63) // 64 * 64), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def flat(name):
        return agg.SendGradients(ipls.DeviceBuffer.from_tensor(src[name]), parts, 7, origin=origin, out=out.data_ptr(),
                                 out_cap=out.numel())

    def frames():
        return agg.publish_partials(parts, 7, parts, origin=origin, target=ipls.TGT_WEIGHTS, out=out.data_ptr(),
                                    out_cap=out.numel())

    def three_step(name):
        buf = ipls.DeviceBuffer.from_tensor(src[name])
        texts = []
        split = agg.OrganizeGradients(buf)
        for p in parts:
            texts.append(base64.urlsafe_b64encode(ipls.frame_encode(split[p], p, 7, 3, origin)))
        return texts

    # the texts agree, once
    ref = three_step("flat_f32")
    lens, offs = flat("flat_f32")
    agg.sync()
    host = out.cpu().numpy()
    for p in parts:
        assert host[offs[p]:offs[p] + lens[p]].tobytes() == ref[p], f"flat_f32 text {p} differs from the three-step route"
    del host, ref

    legs = ["flat_f64", "flat_f32", "flat_bf16", "frames"]
    run = {k: (lambda k=k: flat(k)) for k in legs[:3]}
    run["frames"] = frames
    for k in legs:
        run[k]()
    agg.sync()
    times = {k: [] for k in legs + ["three_step"]}
    for rep in range(a.reps):
        order = legs[rep % len(legs):] + legs[:rep % len(legs)]       # rotate: no leg always follows the same one
        for k in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run[k]()
            e1.record(stream)
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
        if rep < a.host_reps:
            t0 = time.perf_counter()
            three_step("flat_f64")
            times["three_step"].append(1e3 * (time.perf_counter() - t0))
    values = P * L
    res = {"parts": P, "len": L, "reps": a.reps, "origin_len": len(origin), "load_form": "element loads", "legs": {}}
    for k, ts in times.items():
        if not ts:
            continue
        per_value = {"frames": 8 + 32 / 3, "three_step": None}.get(k, esize.get(k, 0) + 32 / 3)
        med = statistics.median(ts)
        res["legs"][k] = {"ms": [round(t, 4) for t in ts], "min_ms": round(min(ts), 4), "median_ms": round(med, 4),
                          "max_ms": round(max(ts), 4),
                          "gbps_median": None if per_value is None else round(values * per_value / med / 1e6, 1)}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    agg.close()


if __name__ == "__main__":
    main()
