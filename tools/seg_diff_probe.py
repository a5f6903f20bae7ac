"""The trainer's update as a difference of two tensor lists against the route
a PyTorch caller had before it, written to
profiles/seg_diff/probe.json.

Two pairs of parameter lists, seeded: about 64 Mi values in about 150 tensors
of 1 Ki to 4 Mi elements, once all float32 and once as bfloat16 matrices with
float32 vectors; the received model and the trained parameters (the model plus
a small step).  The handle has P = 16 partitions.  Two workloads:

  update  all partitions owned.
  round   half the partitions owned, the other half sent (SendGradients into a
          device text buffer).

Routes: `diff` is UpdateGradient / SendGradients over ipls.Difference.  The
parent route makes the third list first and hands it to the Segments calls,
in the faster of two ways, both timed: `foreach` is torch._foreach_sub (a new
list every call), `sub_out` is torch.sub(out=) per tensor into a preallocated
list.  The parent route of the result is the faster of the two, named in
`parent_route`.

Everything runs in one process on the handle's own stream (torch's work too,
through torch.cuda.ExternalStream).  Every shape is warmed up first and the
outputs of all routes are compared bit for bit at the timed size.  A span is
timed with device events around at least --span seconds of back-to-back calls;
the routes alternate, 5 spans each, and the parent route is then run against
itself: `aa_spread` is the largest relative difference between neighbouring
spans of the same route.  Bytes moved are counted, not measured.
Run on the GPU:  python tools/seg_diff_probe.py [--out DIR] [--span 0.5]
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


def sizes(rng, count, lo, hi, target):
    """`count` sizes, log-uniform in [lo, hi], scaled towards `target` values in all."""
    n = np.exp(rng.uniform(np.log(lo), np.log(hi), count))
    for _ in range(8):
        n = np.clip(n * (target / n.sum()), lo, hi)
    return [int(x) for x in n]


def make_lists(name, seed):
    """(received model, trained parameters): the same shapes and dtypes."""
    rng = np.random.default_rng(seed)
    ns = sizes(rng, 150, 1 << 10, 4 << 20, 64 << 20)
    g = torch.Generator(device="cuda").manual_seed(seed)
    model, trained = [], []
    for n in ns:
        dt = torch.bfloat16 if name == "150xmixed" and n >= (64 << 10) else torch.float32
        w = torch.randn(n, device="cuda", generator=g) * 1e-1
        step = torch.randn(n, device="cuda", generator=g) * 1e-3
        model.append(w.to(dt))
        trained.append((w - step).to(dt))
    return model, trained


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


def compare(stream, routes, span_s, n_spans=5):
    """Alternate the routes, then the faster parent route against itself."""
    for fn in routes.values():
        fn()
    stream.synchronize()
    spans = {k: [] for k in routes}
    for _ in range(n_spans):
        for k, fn in routes.items():
            spans[k].append(timed(stream, fn, span_s))
    out = {k: {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v), "spans_s": v}
           for k, v in spans.items()}
    parent = min((k for k in routes if k != "diff"), key=lambda k: out[k]["median_s"])
    aa = [timed(stream, routes[parent], span_s) for _ in range(2 * n_spans)]
    out["parent_route"] = parent
    out["aa_spread"] = max(abs(x - y) / min(x, y) for x, y in zip(aa, aa[1:]))
    out["aa_spans_s"] = aa
    return out


def probe(name, span_s):
    model, trained = make_lists(name, 20261)
    M = sum(t.numel() for t in model)
    src_bytes = sum(t.numel() * t.element_size() for t in model)    # s per value, summed
    res = {"list": name, "tensors": len(model), "values": M, "partitions": P, "source_bytes": src_bytes,
           "workloads": {}}
    own_all, own_half, sent = list(range(P)), list(range(0, P, 2)), list(range(1, P, 2))
    with ipls.Aggregator(model_size=M, n_partitions=P) as A, ipls.Aggregator(model_size=M, n_partitions=P) as B, \
            ipls.Aggregator(model_size=M, n_partitions=P) as C:
        sa, sb, sc = (torch.cuda.ExternalStream(h.stream) for h in (A, B, C))
        diff = ipls.Difference(model, trained)
        outs = [torch.empty_like(t) for t in model]
        oseg = ipls.Segments.from_tensors(outs)
        text_cap = sum((((14 + 8 * A.lengths[p]) + 2) // 3 * 4 + 63) // 64 * 64 for p in sent) + 64
        texts = [torch.zeros(text_cap, dtype=torch.uint8, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()

        def foreach():
            return ipls.Segments.from_tensors(torch._foreach_sub(model, trained))

        def sub_out():
            for a, b, o in zip(model, trained, outs):
                torch.sub(a, b, out=o)
            return oseg

        def round_of(agg, make, text):
            seg = make()
            agg.UpdateGradient(seg, own_half)
            agg.SendGradients(seg, sent, 7, out=text.data_ptr(), out_cap=text_cap)

        # ---- the outputs of the three routes, bit for bit, at the timed size ----
        for agg, st, make, text in ((A, sa, foreach, texts[0]), (B, sb, sub_out, texts[1]),
                                    (C, sc, lambda: diff, texts[2])):
            with torch.cuda.stream(st):
                agg.UpdateGradient(make(), own_all)
                round_of(agg, make, text)
        A.sync(), B.sync(), C.sync()
        same = all(A.checksum(p) == B.checksum(p) == C.checksum(p) for p in range(P))
        same = same and torch.equal(texts[0], texts[2]) and torch.equal(texts[1], texts[2])
        res["outputs_bit_identical"] = bool(same)
        if not same:
            return res

        # ---- timing: one handle, one stream.  Bytes by count, s = bytes per source value:
        # the subtraction 3 s, the own-accumulate s + 16 (2 s + 16 from two lists), the send s + 32/3 (2 s + 32/3)
        work = {
            "update": ({"foreach": lambda: A.UpdateGradient(foreach(), own_all),
                        "sub_out": lambda: A.UpdateGradient(sub_out(), own_all),
                        "diff": lambda: A.UpdateGradient(diff, own_all)},
                       {"parent": 4 * src_bytes + 16 * M, "diff": 2 * src_bytes + 16 * M}),
            "round": ({"foreach": lambda: round_of(A, foreach, texts[0]),
                       "sub_out": lambda: round_of(A, sub_out, texts[0]),
                       "diff": lambda: round_of(A, lambda: diff, texts[0])},
                      {"parent": 4 * src_bytes + (16 * M + 32 * M // 3) // 2,
                       "diff": 2 * src_bytes + (16 * M + 32 * M // 3) // 2}),
        }
        with torch.cuda.stream(sa):
            for wname, (routes, nbytes) in work.items():
                r = compare(sa, routes, span_s)
                parent = r["parent_route"]
                r["bytes_by_count"] = nbytes
                r["bytes_ratio_by_count"] = nbytes["diff"] / nbytes["parent"]
                r["diff_GBps_by_count"] = nbytes["diff"] / r["diff"]["median_s"] / 1e9
                r["parent_GBps_by_count"] = nbytes["parent"] / r[parent]["median_s"] / 1e9
                r["diff_over_parent"] = r["diff"]["median_s"] / r[parent]["median_s"]
                r["not_slower_within_spread"] = r["diff"]["median_s"] <= r[parent]["median_s"] * (1 + r["aa_spread"])
                res["workloads"][wname] = r
                print(name, wname, json.dumps({k: r[k] for k in ("parent_route", "diff_over_parent", "aa_spread",
                                                                 "not_slower_within_spread")}),
                      {k: round(1e3 * r[k]["median_s"], 3) for k in routes}, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "seg_diff"))
    ap.add_argument("--span", type=float, default=0.5)
    ap.add_argument("--lists", default="150xf32,150xmixed")
    a = ap.parse_args()
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "span_s": a.span, "build": ipls.build_info(), "lists": []}
    for name in a.lists.split(","):
        res["lists"].append(probe(name, a.span))
        torch.cuda.empty_cache()
    (out / "probe.json").write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", out / "probe.json")


if __name__ == "__main__":
    main()
