"""Measurements of the whole-gradient streamed update, written
under profiles/update_flat/.  One leg per run:

  --leg kernel    kernel.txt: tools/update_flat_sweep.hip (make -C
                  ipls-java-api_amd sweeps): k_update_flat alone against the
                  per-partition k_split launches, its shifted-load form against
                  the element-load form
  --leg call      call.json: the call with a no-op source against the two
                  routes a caller has without it -- UpdateGradient of the whole
                  received vector, and one UpdateChunked per partition -- for
                  big-endian doubles and floats, beside the direct pinned H2D
                  rate of the same process.  With --parent-lib PATH (a build of
                  the parent commit's library) the two older routes are also
                  run in child processes that alternate between that library
                  and this tree's (call_alternating.json)
  --leg chunks    call_chunks.txt: the call at call chunks of 2^19 and 2^21
                  values, even and odd partition stride, f32 / BE / bf16
  --leg loopback  loopback.json: the Middleware loopback socket through the
                  Python server with unit_updates off and on, and the socket
                  alone (the ceiling of bench.py's Middleware leg), the three
                  alternating round by round in one process
  --leg pmc       pmc_<COUNTER>.csv from the counter_collection.csv files that
                  `rocprofv3 --pmc <COUNTER> --output-format csv -- update_flat_sweep 1`
                  left under --pmc-dir: the rows of k_update_flat, per kernel
                  and grid the launches and the first, smallest and largest

Every timing is the median of 7 spans (min and max kept).  Run on the GPU:
    python tools/update_flat_probe.py --leg LEG [--out DIR]
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "ipls-java-api_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
NEW_CALL = "ipls_agg_update_gradient_chunked"


def spans(fn, sync, n=7, inner=3):
    fn()
    sync()
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        sync()
        out.append((time.perf_counter() - t0) / inner)
    return {"median_s": statistics.median(out), "min_s": min(out), "max_s": max(out)}


def noop(dst, off, n):
    return True


def kernel_leg(out):
    exe = ROOT / "ipls-java-api_amd" / "lib" / "update_flat_sweep"
    r = subprocess.run([str(exe)], capture_output=True, text=True, check=True)
    (out / "kernel.txt").write_text(r.stdout)
    print(r.stdout)


def call_leg(M, P, new_call=True):
    """The call legs of one process; new_call=False for a library without the call."""
    import numpy as np
    import torch
    import ipls
    res = {"values": M, "partitions": P, "chunk_values": M // P + 1, "library": os.environ.get("IPLS_AGG_LIB", "in-tree"),
           "legs": {}}
    pinned = torch.zeros(8 * M, dtype=torch.uint8).pin_memory()
    dev = torch.empty(8 * M, dtype=torch.uint8, device="cuda")
    h2d = spans(lambda: dev.copy_(pinned, non_blocking=True), torch.cuda.synchronize)
    res["pinned_h2d_GBps"] = 8 * M / h2d["median_s"] / 1e9
    del dev
    host = pinned.numpy()
    for name, kw, s in (("HOST_BE", dict(big_endian=True), 8), ("HOST_F32", dict(dtype=np.float32), 4)):
        with ipls.Aggregator(model_size=M, n_partitions=P) as agg:
            vec = host[:s * M] if s == 8 else host[:4 * M].view(np.float32)
            legs = {
                "receive_then_update_gradient": lambda: agg.UpdateGradient(vec, range(P)),
                "P_accumulate_chunked": lambda: [agg.UpdateChunked(p, agg.lengths[p], noop, **kw) for p in range(P)],
            }
            if new_call:
                legs["update_gradient_chunked"] = lambda: agg.UpdateGradientChunked(M, noop, range(P), **kw)
            for leg, fn in legs.items():
                r = spans(fn, agg.sync)
                r["values_per_s"] = M / r["median_s"]
                r["GBps"] = s * M / r["median_s"] / 1e9
                res["legs"][f"{name}/{leg}"] = r
                print(name, leg, json.dumps(r), flush=True)
    return res


def alternating(a, out):
    """The legs both libraries can run, in child processes new, parent, new, parent."""
    runs = []
    for i in range(4):
        which = "parent" if i % 2 else "new"
        env = dict(os.environ)
        if which == "parent":
            env["IPLS_AGG_LIB"] = str(Path(a.parent_lib).resolve())
        cmd = [sys.executable, __file__, "--leg", "call-child", "--values", str(a.values), "--partitions", str(a.partitions)]
        r = subprocess.run(cmd + (["--without-new-call"] if which == "parent" else []), env=env, capture_output=True,
                           text=True, check=True)
        res = json.loads(r.stdout.strip().splitlines()[-1])
        res["library"] = which
        runs.append(res)
        print(which, json.dumps({k: round(1e3 * v["median_s"], 3) for k, v in res["legs"].items()}), flush=True)
    (out / "call_alternating.json").write_text(json.dumps(runs, indent=1) + "\n")


def chunks_leg(a, out):
    import numpy as np
    import ipls
    P = a.partitions
    lines = [f"# UpdateGradientChunked, a source that returns at once, {P} partitions, one process, two rounds:",
             "# even and odd partition stride (chunk rule); f32, big-endian f64, bf16; call chunks of 2^19 and",
             "# 2^21 values; median / min / max of 7 spans of 3 calls, a handle sync per span"]
    for rnd in range(2):
        for M in (a.values - P, a.values + 5):
            with ipls.Aggregator(model_size=M, n_partitions=P) as agg:
                for name, kw in (("f32", dict(dtype=np.float32)), ("be", dict(big_endian=True)), ("bf16", dict(dtype="bf16"))):
                    for chunk in (1 << 19, 1 << 21):
                        r = spans(lambda: agg.UpdateGradientChunked(M, noop, range(P), chunk=chunk, **kw), agg.sync)
                        lines.append(f"{rnd} chunk rule {M // P + 1} {name} call chunk {chunk} median "
                                     f"{1e3 * r['median_s']:.2f} min {1e3 * r['min_s']:.2f} max {1e3 * r['max_s']:.2f} ms")
                        print(lines[-1], flush=True)
    (out / "call_chunks.txt").write_text("\n".join(lines) + "\n")


def loopback_leg(a, out):
    """bench.py's Middleware leg with a second server: K task-2 updates of M
    doubles and one task-3 reply per round over TCP 127.0.0.1, against the
    socket alone (one pinned buffer, no aggregator), the per-partition server
    and the unit server, one cold round of each and then warm rounds that
    alternate ceiling / off / on."""
    import socket
    import struct
    import threading
    import numpy as np
    import ipls
    from ipls import middleware as MW
    M, P, K, D, warm = a.values, a.partitions, a.updates, 2, a.rounds
    nbytes = 8 * M
    rng = np.random.default_rng(7)
    ups = [rng.standard_normal(M).astype(">f8").view(np.uint8) for _ in range(D)]
    replies = {k: np.zeros(nbytes, dtype=np.uint8) for k in ("off", "on", "ceiling")}
    hdr2, hdr3 = struct.pack(">h", 2), struct.pack(">h", 3)

    def task(port, hdr, payload, n_reply, into=None):
        with socket.create_connection(("127.0.0.1", port)) as s:
            s.sendall(hdr)
            if payload is not None:
                s.sendall(memoryview(payload))
            return MW._recv_exact(s, n_reply, into)

    def one_round(port, reply):
        t2 = []
        t0 = time.perf_counter()
        for k in range(K):
            t = time.perf_counter()
            assert bytes(task(port, hdr2, ups[k % D], 2)) == MW.ACK
            t2.append(time.perf_counter() - t)
        t = time.perf_counter()
        task(port, hdr3, None, nbytes, reply)
        t3 = time.perf_counter() - t
        dt = time.perf_counter() - t0
        return {"seconds": dt, "GBps": (K + 1) * nbytes / dt / 1e9, "task2_ms_median": 1e3 * statistics.median(t2),
                "task2_ms_min": 1e3 * min(t2), "task2_ms_max": 1e3 * max(t2), "task3_ms": 1e3 * t3}

    n_rounds = 1 + warm
    staging = ipls.PinnedBuffer(nbytes)
    staging.view()[::4096] = 0
    srv = socket.socket()
    srv.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
    srv.bind(("127.0.0.1", 0))
    srv.listen(16)

    def null_server(n_conn):
        for _ in range(n_conn):
            conn, _ = srv.accept()
            with conn:
                (t,) = struct.unpack(">h", MW._recv_exact(conn, 2))
                if t == 2:
                    MW._recv_exact(conn, nbytes, staging.view())
                    conn.sendall(MW.ACK)
                elif t == 3:
                    conn.sendall(memoryview(staging.view())[:nbytes])
    threads = [threading.Thread(target=null_server, args=(n_rounds * (K + 1),), daemon=True)]
    ports = {"ceiling": srv.getsockname()[1]}
    opts = MW.parse_arguments(f"-p 0 -pa {P} -mp 1 -n {K} -i 0 -training 0 -aggr 0".split())
    for name, unit in (("off", False), ("on", True)):
        got, ready = [], threading.Event()
        threads.append(threading.Thread(target=MW.serve, daemon=True, kwargs=dict(
            opts=opts, max_connections=1 + n_rounds * (K + 1), ready=ready, on_listen=got.append, unit_updates=unit)))
        threads[-1].start()
        assert ready.wait(60), "the middleware server did not start"
        ports[name] = got[0]
        assert bytes(task(got[0], MW.encode_init(False, [], "/ip4/127.0.0.1/tcp/5001", "probe", M), None, 2)) == MW.ACK
    threads[0].start()
    rounds = []
    for r in range(n_rounds):
        rounds.append({name: one_round(ports[name], replies[name]) for name in ("ceiling", "off", "on")})
        print(r, json.dumps({k: round(v["GBps"], 3) for k, v in rounds[-1].items()}), flush=True)
    for th in threads:
        th.join(120)
    srv.close()
    staging.close()
    same = bool(np.array_equal(replies["off"], replies["on"]))
    res = {"values": M, "partitions": P, "updates_per_round": K, "MB_per_task": nbytes / 1e6, "cold_round": rounds[0],
           "warm_rounds": rounds[1:], "replies_identical": same}
    for name in ("off", "on"):
        fr = [r[name]["GBps"] / r["ceiling"]["GBps"] for r in rounds[1:]]
        res[f"unit_{name}"] = {"frac_of_ceiling_per_round": fr, "frac_of_ceiling_median": statistics.median(fr),
                               "GBps_median": statistics.median(r[name]["GBps"] for r in rounds[1:]),
                               "task2_ms_median": statistics.median(r[name]["task2_ms_median"] for r in rounds[1:])}
    res["ceiling_GBps_median"] = statistics.median(r["ceiling"]["GBps"] for r in rounds[1:])
    res["ceiling_task2_ms_median"] = statistics.median(r["ceiling"]["task2_ms_median"] for r in rounds[1:])
    (out / "loopback.json").write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: res[k] for k in ("unit_off", "unit_on", "ceiling_GBps_median", "replies_identical")}))
    assert same, "the two servers answered task 3 differently"


def pmc_leg(a, out):
    """Condense rocprofv3's per-dispatch counter rows to one row per kernel and grid."""
    groups = {}
    for f in sorted(Path(a.pmc_dir).rglob("*counter_collection.csv")):
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                if "k_update_flat" not in row["Kernel_Name"]:
                    continue
                key = (row["Counter_Name"], row["Kernel_Name"][:70], int(row["Grid_Size"]))
                groups.setdefault(key, []).append(float(row["Counter_Value"]))
    for counter in sorted({k[0] for k in groups}):
        with open(out / f"pmc_{counter}.csv", "w", newline="") as fh:
            w = csv.writer(fh)
            w.writerow(["kernel", "grid", "launches", "counter", "first_KiB", "min_KiB", "max_KiB"])
            for (c, kernel, grid), v in sorted(groups.items(), key=lambda kv: (kv[0][2], kv[0][1])):
                if c == counter:
                    w.writerow([kernel, grid, len(v), c, f"{v[0]:.2f}", f"{min(v):.2f}", f"{max(v):.2f}"])
        print("wrote", out / f"pmc_{counter}.csv")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=("kernel", "call", "call-child", "chunks", "loopback", "pmc"))
    ap.add_argument("--values", type=int, default=64 << 20)
    ap.add_argument("--partitions", type=int, default=16)
    ap.add_argument("--updates", type=int, default=8, help="task-2 updates per loopback round")
    ap.add_argument("--rounds", type=int, default=5, help="warm loopback rounds")
    ap.add_argument("--parent-lib", help="a build of the parent commit's library, for the alternating call legs")
    ap.add_argument("--without-new-call", action="store_true")
    ap.add_argument("--pmc-dir", help="where rocprofv3 left its counter_collection.csv files")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "update_flat"))
    a = ap.parse_args()
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    if a.leg == "kernel":
        kernel_leg(out)
    elif a.leg == "call-child":
        if a.without_new_call:   # the parent's library has no such symbol to bind
            from ipls import _native as N
            N.SIGNATURES.pop(NEW_CALL, None)
        print(json.dumps(call_leg(a.values + 5, a.partitions, new_call=not a.without_new_call)))
    elif a.leg == "call":
        res = call_leg(a.values + 5, a.partitions)    # an odd chunk: M / P + 1 = 2^k / P + 1
        (out / "call.json").write_text(json.dumps(res, indent=1) + "\n")
        if a.parent_lib:
            alternating(a, out)
    elif a.leg == "chunks":
        chunks_leg(a, out)
    elif a.leg == "loopback":
        loopback_leg(a, out)
    elif a.leg == "pmc":
        pmc_leg(a, out)


if __name__ == "__main__":
    main()
