"""K trainers' tensor lists folded by one call against the K calls it replaces
(DESIGN.md §3.9), written to profiles/seg_peers/probe.json.

Seeded lists: 2^24 values in 150 tensors of 256 to 1 Mi elements, once all
float32 and once as bfloat16 matrices with float32 vectors; one received model
and 32 sets of trained parameters (the model plus a small step each).  The
handle has P = 16 partitions, all owned.  For K in 1, 8, 32:

  peers   one UpdateGradient over ipls.PeerUpdates(trained[:K], received);
  parent  K calls UpdateGradient(ipls.Difference(received, trained[k])), which
          is what a caller had before; at K = 1 it is the single-peer twin.

Everything runs in one process on the handle's own stream.  Every shape is
warmed up first and the accumulators of both routes are compared by checksum
at the timed size.  A span is timed with device events around at least --span
seconds of back-to-back calls; the routes alternate, 5 spans each, and the
parent route is then run against itself: `aa_spread` is the largest relative
difference between neighbouring spans of that one route.  These are spans of
whole calls (host plan, table upload, launch and kernel), not kernel-only
times.  Bytes moved are counted, not measured.

--groups LIB2,LIB4,LIB8: builds of the library with 2, 4 and 8 peers' loads in
flight (make peers_groups); each is timed in a child process of its own, the
peers route alone, and the medians go into `group_sweep`.
Run on the GPU:  python tools/seg_peers_probe.py [--out DIR] [--span 0.5]
"""
import argparse
import json
import os
import statistics
import subprocess
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
KS = (1, 8, 32)
VALUES = 1 << 24


def sizes(rng, count, lo, hi, target):
    """`count` sizes, log-uniform in [lo, hi], scaled towards `target` values in all."""
    n = np.exp(rng.uniform(np.log(lo), np.log(hi), count))
    for _ in range(8):
        n = np.clip(n * (target / n.sum()), lo, hi)
    return [int(x) for x in n]


def make_lists(name, seed, k_max):
    """(received model, k_max lists of trained parameters): the same shapes and dtypes."""
    rng = np.random.default_rng(seed)
    ns = sizes(rng, 150, 1 << 8, 1 << 20, VALUES)
    g = torch.Generator(device="cuda").manual_seed(seed)
    model, trained = [], [[] for _ in range(k_max)]
    for n in ns:
        dt = torch.bfloat16 if name == "150xmixed" and n >= (16 << 10) else torch.float32
        w = torch.randn(n, device="cuda", generator=g) * 1e-1
        model.append(w.to(dt))
        for t in trained:
            t.append((w - torch.randn(n, device="cuda", generator=g) * 1e-3).to(dt))
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


def stats(v):
    return {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v), "spans_s": v}


def compare(stream, routes, span_s, n_spans=5):
    """Alternate the routes, then the parent route against itself."""
    for fn in routes.values():
        fn()
    stream.synchronize()
    spans = {k: [] for k in routes}
    for _ in range(n_spans):
        for k, fn in routes.items():
            spans[k].append(timed(stream, fn, span_s))
    out = {k: stats(v) for k, v in spans.items()}
    aa = [timed(stream, routes["parent"], span_s) for _ in range(2 * n_spans)]
    out["aa_spread"] = max(abs(x - y) / min(x, y) for x, y in zip(aa, aa[1:]))
    out["aa_spans_s"] = aa
    return out


def probe(name, span_s, peers_only):
    model, trained = make_lists(name, 20262, max(KS))
    M = sum(t.numel() for t in model)
    src_bytes = sum(t.numel() * t.element_size() for t in model)    # s per value, summed
    res = {"list": name, "tensors": len(model), "values": M, "partitions": P, "source_bytes": src_bytes, "peers": {}}
    own = list(range(P))
    with ipls.Aggregator(model_size=M, n_partitions=P) as A, ipls.Aggregator(model_size=M, n_partitions=P) as B:
        sa = torch.cuda.ExternalStream(A.stream)
        diffs = [ipls.Difference(model, t) for t in trained]
        torch.cuda.synchronize()
        for K in KS:
            pu = ipls.PeerUpdates(trained[:K], received=model)

            def peers(agg=A):
                agg.UpdateGradient(pu, own)

            def parent(agg=A):
                for d in diffs[:K]:
                    agg.UpdateGradient(d, own)

            # ---- the accumulators of both routes at the timed size: from zeros, then into the result ----
            A.reset(), B.reset()
            for _ in range(2):
                peers(A), parent(B)
            A.sync(), B.sync()
            same = all(A.checksum(p) == B.checksum(p) for p in range(P))
            r = {"outputs_bit_identical": bool(same), "launch": A.last_launch()}
            res["peers"][str(K)] = r
            if not same:
                continue
            with torch.cuda.stream(sa):
                if peers_only:
                    peers()
                    sa.synchronize()
                    r["peers"] = stats([timed(sa, peers, span_s) for _ in range(5)])
                    continue
                r.update(compare(sa, {"peers": peers, "parent": parent}, span_s))
            nbytes = {"peers": (K + 1) * src_bytes + 16 * M, "parent": K * (2 * src_bytes + 16 * M)}
            r["bytes_by_count"] = nbytes
            r["bytes_ratio_by_count"] = nbytes["peers"] / nbytes["parent"]
            r["peers_GBps_by_count"] = nbytes["peers"] / r["peers"]["median_s"] / 1e9
            r["parent_GBps_by_count"] = nbytes["parent"] / r["parent"]["median_s"] / 1e9
            r["peers_over_parent"] = r["peers"]["median_s"] / r["parent"]["median_s"]
            r["not_slower_within_spread"] = r["peers"]["median_s"] <= r["parent"]["median_s"] * (1 + r["aa_spread"])
            print(name, "K", K, json.dumps({k: r[k] for k in ("peers_over_parent", "bytes_ratio_by_count", "aa_spread",
                                                              "not_slower_within_spread")}),
                  {k: round(1e3 * r[k]["median_s"], 3) for k in ("peers", "parent")}, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "seg_peers"))
    ap.add_argument("--span", type=float, default=0.5)
    ap.add_argument("--lists", default="150xf32,150xmixed")
    ap.add_argument("--groups", default="", help="libraries built with 2, 4 and 8 peers in flight, comma-separated")
    ap.add_argument("--peers-only", action="store_true", help="a leg of the group sweep: print the result, write nothing")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "span_s": a.span, "build": ipls.build_info(), "lists": []}
    for name in a.lists.split(","):
        res["lists"].append(probe(name, a.span, a.peers_only))
        torch.cuda.empty_cache()
    if a.peers_only:
        print("LEG " + json.dumps(res["lists"]))
        return
    if a.groups:
        res["group_sweep"] = {}
        for g, lib in zip((2, 4, 8), a.groups.split(",")):
            env = dict(os.environ, IPLS_AGG_LIB=str(Path(lib).resolve()))
            leg = subprocess.run([sys.executable, __file__, "--peers-only", "--span", str(a.span), "--lists", a.lists],
                                 env=env, capture_output=True, text=True, timeout=600)
            if leg.returncode:
                print(leg.stdout[-2000:], leg.stderr[-2000:])
                raise SystemExit(f"group {g}: leg ended with {leg.returncode}")
            lists = json.loads([ln for ln in leg.stdout.splitlines() if ln.startswith("LEG ")][-1][4:])
            res["group_sweep"][str(g)] = {
                x["list"]: {K: {"median_ms": 1e3 * v["peers"]["median_s"], "bit_identical": v["outputs_bit_identical"]}
                            for K, v in x["peers"].items()} for x in lists}
            print("group", g, json.dumps(res["group_sweep"][str(g)]), flush=True)
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / "probe.json").write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", out / "probe.json")


if __name__ == "__main__":
    main()
