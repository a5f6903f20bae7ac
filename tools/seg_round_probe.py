"""The many-trainers round by one call against the three calls it replaces
(DESIGN.md §3.11), written to profiles/seg_round/probe.json.

Seeded shapes: 2^24 values in 150 tensors of 256 to 1 Mi elements, once all
float32 and once as bfloat16 matrices with float32 vectors; a received model
and K trainers' parameters of them, K in 1, 8, 32.  The handle has P = 16
partitions, all owned, AGG and REP logically zero at every call.  The outputs
are the inputs (in place): the received model and every trainer take the new
model.

  fused   one round_peers(peers, all);
  three   UpdateGradient(peers, all), AggregatePartition(ALL_PARTITIONS),
          GetPartitions(out=peers.outputs()).

Everything runs in one process on the handle's own stream.  Every shape is
warmed up first, and W and every list of both routes are compared bit for bit
at the timed size, from the same inputs.  A span is timed with device events
around at least --span seconds of back-to-back calls; the routes alternate, 5
spans each, and the parent route (`three`) is then run against itself:
`aa_spread` is the largest relative difference between neighbouring spans of
that one route.  These are spans of whole calls (host plans, table uploads,
launches and kernels), not kernel-only times.  Bytes moved are counted, not
measured.
Run on the GPU:  python tools/seg_round_probe.py [--out DIR] [--span 0.5]
The kernel's other forms at misaligned lists (element loads and stores for
every format; shifted vectors for every format) are build variants,
`make -C ipls-java-api_amd round_variants`; the same probe on each:
  IPLS_AGG_LIB=ipls-java-api_amd/lib/ab/libipls_agg_roundshift0.so \
      python tools/seg_round_probe.py --name probe_shift0.json      (and 2)
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
KS = (1, 8, 32)
VALUES = 1 << 24
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def sizes(rng, count, lo, hi, target):
    """`count` sizes, log-uniform in [lo, hi], scaled towards `target` values in all."""
    n = np.exp(rng.uniform(np.log(lo), np.log(hi), count))
    for _ in range(8):
        n = np.clip(n * (target / n.sum()), lo, hi)
    return [int(x) for x in n]


def make_lists(name, seed, n_lists):
    """n_lists lists of tensors of the same shapes and dtypes: small normals, a different stream per list."""
    rng = np.random.default_rng(seed)
    ns = sizes(rng, 150, 1 << 8, 1 << 20, VALUES)
    dts = [torch.bfloat16 if name == "150xmixed" and n >= (16 << 10) else torch.float32 for n in ns]
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return [[torch.randn(n, dtype=torch.float32, device="cuda", generator=g).to(dt) for n, dt in zip(ns, dts)]
            for _ in range(n_lists)]


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


def compare(stream, routes, parent, span_s, n_spans=5):
    """Alternate the routes, then the parent route against itself."""
    for fn in routes.values():
        fn()
    stream.synchronize()
    spans = {k: [] for k in routes}
    for _ in range(n_spans):
        for k, fn in routes.items():
            spans[k].append(timed(stream, fn, span_s))
    out = {k: stats(v) for k, v in spans.items()}
    aa = [timed(stream, routes[parent], span_s) for _ in range(2 * n_spans)]
    out["aa_spread"] = max(abs(x - y) / min(x, y) for x, y in zip(aa, aa[1:]))
    out["aa_spans_s"] = aa
    return out


def same_bits(a, b):
    return all(torch.equal(x.view(BITS[x.dtype]), y.view(BITS[y.dtype])) for x, y in zip(a, b))


def probe(name, span_s, ks=KS):
    lists = make_lists(name, 20264, max(ks) + 1)
    M = sum(t.numel() for t in lists[0])
    s_bytes = sum(t.numel() * t.element_size() for t in lists[0])    # s per value, summed
    res = {"list": name, "tensors": len(lists[0]), "values": M, "partitions": P, "list_bytes": s_bytes, "K": {}}
    owned = list(range(P))
    with ipls.Aggregator(model_size=M, n_partitions=P) as A:
        sa = torch.cuda.ExternalStream(A.stream)
        torch.cuda.synchronize()
        for K in ks:
            pu = ipls.PeerUpdates(lists[1:K + 1], received=lists[0])
            out = pu.outputs()

            def fused():
                A.round_peers(pu, owned, out=out)

            def three():
                A.UpdateGradient(pu, owned)
                A.AggregatePartition(ipls.ALL_PARTITIONS)
                A.GetPartitions(out=out)

            routes = {"fused": fused, "three": three}
            # ---- W and every list of both routes, bit for bit, at the timed size, from the same inputs ----
            with torch.cuda.stream(sa):
                saved = [[t.clone() for t in x] for x in lists[:K + 1]]
                sa.synchronize()
                three()
                sa.synchronize()
                ref = [[t.clone() for t in x] for x in lists[:K + 1]]
                w_ref = [A.read(p, ipls.TGT_WEIGHTS).view(np.uint64).copy() for p in range(P)]
                for x, y in zip(lists[:K + 1], saved):
                    torch._foreach_copy_(x, y)
                sa.synchronize()
                fused()
                sa.synchronize()
                same = {"lists": all(same_bits(x, y) for x, y in zip(lists[:K + 1], ref)),
                        "W": all(np.array_equal(A.read(p, ipls.TGT_WEIGHTS).view(np.uint64), w_ref[p]) for p in range(P)),
                        "changed": not all(same_bits(x, y) for x, y in zip(lists[:K + 1], saved))}
                del ref, saved
            r = {"bit_identical": same, "launch": A.last_launch()}
            res["K"][str(K)] = r
            if not all(same.values()):
                continue
            with torch.cuda.stream(sa):
                r.update(compare(sa, routes, "three", span_s))
            # AGG and REP logically zero, all partitions owned, K + 1 lists written
            nbytes = {"fused": s_bytes + K * s_bytes + 8 * M + (K + 1) * s_bytes,
                      "three": (s_bytes + K * s_bytes + 8 * M) + 16 * M + (8 * M + (K + 1) * s_bytes)}
            r["bytes_by_count"] = nbytes
            r["bytes_ratio_by_count"] = nbytes["fused"] / nbytes["three"]
            r["GBps_by_count"] = {k: nbytes[k] / r[k]["median_s"] / 1e9 for k in routes}
            r["fused_over_three"] = r["fused"]["median_s"] / r["three"]["median_s"]
            r["not_slower_within_spread"] = r["fused"]["median_s"] <= r["three"]["median_s"] * (1 + r["aa_spread"])
            print(name, "K", K, json.dumps({k: r[k] for k in ("fused_over_three", "bytes_ratio_by_count", "aa_spread",
                                                              "not_slower_within_spread")}),
                  {k: round(1e3 * r[k]["median_s"], 3) for k in routes}, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "seg_round"))
    ap.add_argument("--span", type=float, default=0.5)
    ap.add_argument("--lists", default="150xf32,150xmixed")
    ap.add_argument("--ks", default=",".join(str(k) for k in KS))
    ap.add_argument("--name", default="probe.json", help="the file written under --out")
    a = ap.parse_args()
    from ipls import _native
    res = {"device": torch.cuda.get_device_name(0), "span_s": a.span, "build": ipls.build_info(),
           "library": Path(_native.LIB_PATH).name, "lists": []}
    for name in a.lists.split(","):
        res["lists"].append(probe(name, a.span, tuple(int(k) for k in a.ks.split(","))))
        torch.cuda.empty_cache()
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / a.name).write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", out / a.name)


if __name__ == "__main__":
    main()
