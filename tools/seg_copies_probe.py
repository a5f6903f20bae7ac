"""GetPartitions into n_lists tensor lists by one call against the two routes a
caller had before, written to profiles/seg_copies/probe.json.

Seeded shapes: 2^24 values in 150 tensors of 256 to 1 Mi elements, once all
float32 and once as bfloat16 matrices with float32 vectors; 33 lists of them
(the received model and 32 trainers' parameters).  The handle has P = 16
partitions with a different count each.  For n_lists in 1, 9, 33:

  copies  one GetPartitions(out=ipls.ModelCopies(lists[:n]));
  calls   n calls GetPartitions(out=ipls.Segments(list k));
  copy    one GetPartitions(out=list 0), then torch._foreach_copy_(list k,
          list 0) for k = 1 .. n - 1, on the handle's stream.

At n_lists = 1 both parent routes are the single-list twin.  Everything runs in
one process on the handle's own stream.  Every shape is warmed up first and
every list of every route is compared bit for bit with the `calls` route's at
the timed size.  A span is timed with device events around at least --span
seconds of back-to-back calls; the routes alternate, 5 spans each, and the
faster parent route is then run against itself: `aa_spread` is the largest
relative difference between neighbouring spans of that one route.  These are
spans of whole calls (host plan, table upload, launch and kernel), not
kernel-only times.  Bytes moved are counted, not measured.
Run on the GPU:  python tools/seg_copies_probe.py [--out DIR] [--span 0.5]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "ipls-java-api_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np   # noqa: E402
import torch         # noqa: E402
import ipls          # noqa: E402

P = 16
NS = (1, 9, 33)
VALUES = 1 << 24
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def sizes(rng, count, lo, hi, target):
    """`count` sizes, log-uniform in [lo, hi], scaled towards `target` values in all."""
    n = np.exp(rng.uniform(np.log(lo), np.log(hi), count))
    for _ in range(8):
        n = np.clip(n * (target / n.sum()), lo, hi)
    return [int(x) for x in n]


def make_lists(name, seed, n_lists):
    """n_lists lists of tensors of the same shapes and dtypes, every element junk."""
    rng = np.random.default_rng(seed)
    ns = sizes(rng, 150, 1 << 8, 1 << 20, VALUES)
    dts = [torch.bfloat16 if name == "150xmixed" and n >= (16 << 10) else torch.float32 for n in ns]
    return [[torch.full((n,), 7.0, dtype=dt, device="cuda") for n, dt in zip(ns, dts)] for _ in range(n_lists)]


def timed(stream, fn, span_s):
    """Seconds per call: device events around enough back-to-back calls to fill span_s."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    reps = max(1, int(span_s / max(a.elapsed_time(b) / 1e3, 1e-6)) + 1)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


def stats(v):
    return {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v), "spans_s": v}


def compare(stream, routes, parents, span_s, n_spans=5):
    """Alternate the routes, then the faster parent route against itself."""
    for fn in routes.values():
        fn()
    stream.synchronize()
    spans = {k: [] for k in routes}
    for _ in range(n_spans):
        for k, fn in routes.items():
            spans[k].append(timed(stream, fn, span_s))
    out = {k: stats(v) for k, v in spans.items()}
    best = min(parents, key=lambda k: out[k]["median_s"])
    aa = [timed(stream, routes[best], span_s) for _ in range(2 * n_spans)]
    out["parent_route"] = best
    out["aa_spread"] = max(abs(x - y) / min(x, y) for x, y in zip(aa, aa[1:]))
    out["aa_spans_s"] = aa
    return out


def same_bits(a, b):
    return all(torch.equal(x.view(BITS[x.dtype]), y.view(BITS[y.dtype])) for x, y in zip(a, b))


def probe(name, span_s):
    lists = make_lists(name, 20263, max(NS))
    M = sum(t.numel() for t in lists[0])
    out_bytes = sum(t.numel() * t.element_size() for t in lists[0])    # s per value, summed
    res = {"list": name, "tensors": len(lists[0]), "values": M, "partitions": P, "list_bytes": out_bytes, "n_lists": {}}
    rng = np.random.default_rng(5)
    with ipls.Aggregator(model_size=M, n_partitions=P) as A:
        for p in range(P):
            w = rng.standard_normal(A.lengths[p])
            w[-1] = float(p + 2)
            A.cache_partition(p, w)
        sa = torch.cuda.ExternalStream(A.stream)
        segs = [ipls.Segments.from_tensors(x) for x in lists]
        torch.cuda.synchronize()
        for n in NS:
            mc = ipls.ModelCopies(segs[:n])

            def copies():
                A.GetPartitions(out=mc)

            def calls():
                for s in segs[:n]:
                    A.GetPartitions(out=s)

            def copy():
                A.GetPartitions(out=segs[0])
                for x in lists[1:n]:
                    torch._foreach_copy_(x, lists[0])

            routes = {"copies": copies, "calls": calls, "copy": copy}
            # ---- every list of every route, bit for bit, at the timed size ----
            same = {}
            with torch.cuda.stream(sa):
                calls()
                sa.synchronize()
                ref = [[t.clone() for t in x] for x in lists[:n]]
                for k in ("copies", "copy"):
                    for x in lists[:n]:
                        for t in x:
                            t.fill_(7.0)
                    routes[k]()
                    sa.synchronize()
                    same[k] = all(same_bits(x, y) for x, y in zip(lists[:n], ref))
                del ref
            r = {"lists_bit_identical": same, "launch": None}
            copies()
            A.sync()
            r["launch"] = A.last_launch()
            res["n_lists"][str(n)] = r
            if not all(same.values()):
                continue
            with torch.cuda.stream(sa):
                r.update(compare(sa, routes, ("calls", "copy"), span_s))
            nbytes = {"copies": 8 * M + n * out_bytes, "calls": n * (8 * M + out_bytes),
                      "copy": 8 * M + out_bytes + (n - 1) * 2 * out_bytes}
            best = r["parent_route"]
            r["bytes_by_count"] = nbytes
            r["bytes_ratio_by_count"] = {k: nbytes["copies"] / nbytes[k] for k in ("calls", "copy")}
            r["GBps_by_count"] = {k: nbytes[k] / r[k]["median_s"] / 1e9 for k in routes}
            r["copies_over_calls"] = r["copies"]["median_s"] / r["calls"]["median_s"]
            r["copies_over_copy"] = r["copies"]["median_s"] / r["copy"]["median_s"]
            r["copies_over_parent"] = r["copies"]["median_s"] / r[best]["median_s"]
            r["not_slower_within_spread"] = r["copies"]["median_s"] <= r[best]["median_s"] * (1 + r["aa_spread"])
            print(name, "n_lists", n, json.dumps({k: r[k] for k in ("parent_route", "copies_over_calls", "copies_over_copy",
                                                                     "bytes_ratio_by_count", "aa_spread",
                                                                     "not_slower_within_spread")}),
                  {k: round(1e3 * r[k]["median_s"], 3) for k in routes}, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "seg_copies"))
    ap.add_argument("--span", type=float, default=0.5)
    ap.add_argument("--lists", default="150xf32,150xmixed")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "span_s": a.span, "build": ipls.build_info(), "lists": []}
    for name in a.lists.split(","):
        res["lists"].append(probe(name, a.span))
        torch.cuda.empty_cache()
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / "probe.json").write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", out / "probe.json")


if __name__ == "__main__":
    main()
