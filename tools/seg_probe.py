"""The trainer boundary over a list of tensors against the flat route a
PyTorch caller had before it, written to
profiles/segs/probe.json.

Three parameter lists, seeded: about 64 Mi values in about 150 tensors of 1 Ki
to 4 Mi elements, once all float32 and once as bfloat16 matrices with float32
vectors; and 4,096 tensors of 1 Ki to 4 Ki elements (float32).  The handle has
P = 16 partitions.  Three workloads:

  update  all partitions owned.  Parent route: torch.cat of the flattened
          tensors (cast to float32 for the mixed list), then UpdateGradient of
          the flat vector.  New route: UpdateGradient(Segments).
  round   half the partitions owned, the other half sent (SendGradients into
          a device text buffer); the parent route builds the flat vector once.
  model   parent route: GetPartitions(out=flat float32) plus a copy into every
          tensor.  New route: GetPartitions(out=Segments).

Everything of one comparison runs in one process on the handle's own stream
(torch's work too, through torch.cuda.ExternalStream, so neither route needs a
host synchronisation between torch and the library).  Every shape is warmed up
first and the outputs of both routes are compared bit for bit at the timed
size.  A span is timed with device events around at least --span seconds of
back-to-back calls; the two routes alternate, and the parent route is also run
against itself: `aa_spread` is the largest relative difference between
neighbouring spans of the same route.  Bytes moved are counted, not measured.
Run on the GPU:  python tools/seg_probe.py [--out DIR] [--span 0.5]
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


def sizes(rng, count, lo, hi, target=None):
    """`count` sizes, log-uniform in [lo, hi]; scaled towards `target` values in all when given."""
    n = np.exp(rng.uniform(np.log(lo), np.log(hi), count))
    if target:
        for _ in range(8):
            n = np.clip(n * (target / n.sum()), lo, hi)
    return [int(x) for x in n]


def make_list(name, seed):
    rng = np.random.default_rng(seed)
    if name == "4096xsmall":
        ns = sizes(rng, 4096, 1 << 10, 4 << 10)
    else:
        ns = sizes(rng, 150, 1 << 10, 4 << 20, 64 << 20)
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for n in ns:
        dt = torch.bfloat16 if name == "150xmixed" and n >= (64 << 10) else torch.float32
        out.append((torch.randn(n, device="cuda", generator=g) * 1e-2).to(dt))
    return out


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
    """Alternate the routes, then the first against itself."""
    for fn in routes.values():
        fn()
    stream.synchronize()
    spans = {k: [] for k in routes}
    for _ in range(n_spans):
        for k, fn in routes.items():
            spans[k].append(timed(stream, fn, span_s))
    first = next(iter(routes))
    aa = [timed(stream, routes[first], span_s) for _ in range(2 * n_spans)]
    spread = max(abs(x - y) / min(x, y) for x, y in zip(aa, aa[1:]))
    out = {k: {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v)} for k, v in spans.items()}
    out["aa_spread"] = spread
    out["aa_spans_s"] = aa
    return out


def probe(name, span_s):
    tensors = make_list(name, 20260)
    M = sum(t.numel() for t in tensors)
    src_bytes = sum(t.numel() * t.element_size() for t in tensors)
    res = {"list": name, "tensors": len(tensors), "values": M, "partitions": P, "workloads": {}}
    own_all, own_half, sent = list(range(P)), list(range(0, P, 2)), list(range(1, P, 2))
    with ipls.Aggregator(model_size=M, n_partitions=P) as A, ipls.Aggregator(model_size=M, n_partitions=P) as B:
        sa, sb = torch.cuda.ExternalStream(A.stream), torch.cuda.ExternalStream(B.stream)
        seg = ipls.Segments.from_tensors(tensors)
        text_cap = sum((((14 + 8 * A.lengths[p]) + 2) // 3 * 4 + 63) // 64 * 64 for p in sent) + 64
        text_a = torch.zeros(text_cap, dtype=torch.uint8, device="cuda")
        text_b = torch.zeros(text_cap, dtype=torch.uint8, device="cuda")
        outs = [torch.empty_like(t) for t in tensors]
        oseg = ipls.Segments.from_tensors(outs)
        flat_out = torch.empty(M, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def cat():
            return torch.cat([t.reshape(-1).float() for t in tensors])

        def parent_update(agg, owned):
            agg.UpdateGradient(ipls.DeviceBuffer.from_tensor(cat()), owned)

        def parent_round(agg, text):
            flat = ipls.DeviceBuffer.from_tensor(cat())
            agg.UpdateGradient(flat, own_half)
            agg.SendGradients(flat, sent, 7, out=text.data_ptr(), out_cap=text_cap)

        def new_round(agg, text):
            agg.UpdateGradient(seg, own_half)
            agg.SendGradients(seg, sent, 7, out=text.data_ptr(), out_cap=text_cap)

        def parent_model(agg, dst):
            agg.GetPartitions(out=ipls.DeviceBuffer.from_tensor(flat_out))
            at = 0
            for t in dst:
                t.copy_(flat_out[at:at + t.numel()])
                at += t.numel()

        # ---- the outputs of both routes, bit for bit, at the timed size ----
        with torch.cuda.stream(sa):
            parent_update(A, own_all)
            parent_round(A, text_a)
        with torch.cuda.stream(sb):
            B.UpdateGradient(seg, own_all)
            new_round(B, text_b)
        A.sync(), B.sync()
        same = all(A.checksum(p) == B.checksum(p) for p in range(P)) and torch.equal(text_a, text_b)
        for agg in (A, B):      # a model to read back: W = AGG with its count slots
            for p in range(P):
                agg.AggregatePartition(p)
        ref = [torch.empty_like(t) for t in tensors]
        with torch.cuda.stream(sa):
            parent_model(A, ref)
        with torch.cuda.stream(sb):
            B.GetPartitions(out=oseg)
        A.sync(), B.sync()
        same = same and all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(ref, outs))
        res["outputs_bit_identical"] = bool(same)
        if not same:
            return res

        # ---- timing: one handle, one stream ----
        f32_cat = src_bytes + 4 * M          # the cat (and cast): read the tensors, write a float32 vector
        work = {
            "update": ({"parent": lambda: parent_update(A, own_all), "segments": lambda: A.UpdateGradient(seg, own_all)},
                       {"parent": f32_cat + 4 * M + 16 * M, "segments": src_bytes + 16 * M}),
            "round": ({"parent": lambda: parent_round(A, text_a), "segments": lambda: new_round(A, text_a)},
                      None),
            "model": ({"parent": lambda: parent_model(A, ref), "segments": lambda: A.GetPartitions(out=oseg)},
                      {"parent": 8 * M + 4 * M + 4 * M + src_bytes, "segments": 8 * M + src_bytes}),
        }
        with torch.cuda.stream(sa):
            for wname, (routes, nbytes) in work.items():
                r = compare(sa, routes, span_s)
                if nbytes:
                    for k in routes:
                        r[k]["bytes_moved"] = nbytes[k]
                        r[k]["GBps"] = nbytes[k] / r[k]["median_s"] / 1e9
                r["segments_over_parent"] = r["segments"]["median_s"] / r["parent"]["median_s"]
                r["not_slower_within_spread"] = r["segments"]["median_s"] <= r["parent"]["median_s"] * (1 + r["aa_spread"])
                res["workloads"][wname] = r
                print(name, wname, json.dumps({k: r[k] for k in ("segments_over_parent", "aa_spread")}),
                      {k: round(1e3 * r[k]["median_s"], 3) for k in routes}, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "segs"))
    ap.add_argument("--span", type=float, default=0.5)
    ap.add_argument("--lists", default="150xf32,150xmixed,4096xsmall")
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
