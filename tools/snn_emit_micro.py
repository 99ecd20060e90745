"""Host against device emission of the kNum SNN edge lists on the bench's
first cfg3 bootstrap (100k cells x 30 PCs, 90k rows with their cells, exact
kNN at k = 20, NUMBER graphs of k = 10 / 15 / 20).

One process, after one warm call of each:
  host    Engine.snn_multi(emit="host")   (device pass + staging, host decode)
  device  Engine.snn_multi(emit="device") (stage, fetch)
  dev     ccg_snn_edges_cells_dev alone, timed with events (count only, and
          count + fill + sort into preallocated lists)
Writes profiles/snn_emit_micro.json (the medians of `reps` runs, the edge
counts, the bytes the fetch copies).  --dev-only runs the device flavour
alone (for a kernel trace).
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from consensusclustr_amd import Engine  # noqa: E402


def med(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def main():
    dev_only = "--dev-only" in sys.argv
    reps = 5
    ks = (10, 15, 20)
    dev = torch.device("cuda", 0)
    N, d, n = 100000, 30, 90000
    pcs, _ = bench.synth_pcs(torch, N, d, 2000, 20241024 + 3, dev)
    boot_np = np.random.default_rng(123).integers(0, N, n).astype(np.int32)
    eng = Engine(0)
    rows = torch.empty((n, d), dtype=torch.float64, device=dev)
    boot = torch.from_numpy(boot_np).to(dev)
    eng.gather_rows_rm_t(pcs, N, d, boot, rows)
    knn = torch.empty((n, 20), dtype=torch.int32, device=dev)
    eng.knn_boot_t(pcs.t().contiguous(), N, d, boot, int(np.unique(boot_np).size), rows, 20, knn)
    torch.cuda.synchronize()
    kn = knn.cpu().numpy()
    out = {"n": n, "ks": list(ks), "reps": reps}

    # the device flavour alone
    info = torch.zeros(3 + len(ks), dtype=torch.int64, device=dev)
    eng.snn_edges_cells_t(knn, ks, [None] * 3, info, cell=boot)
    torch.cuda.synchronize()
    inf = info.cpu().numpy()
    assert inf[1] == 0 and inf[3] > 0, inf
    edges = [int(e) for e in inf[3:]]
    outs = [(torch.empty(e, dtype=torch.int32, device=dev), torch.empty(e, dtype=torch.int32, device=dev),
             torch.empty(e, dtype=torch.float64, device=dev)) for e in edges]
    eng.snn_edges_cells_t(knn, ks, outs, info, cell=boot)
    torch.cuda.synchronize()

    def timed(o):
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.snn_edges_cells_t(knn, ks, o, info, cell=boot)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return med(ts)

    out["dev_count_only_ms"] = timed([None] * 3)
    out["dev_edges_ms"] = timed(outs)
    out["edges"] = edges
    out["class_rows"] = int(inf[2])
    out["classes"] = int(inf[0])
    out["fetch_bytes"] = 16 * sum(edges)
    if dev_only:
        print(json.dumps(out))
        return
    del outs
    torch.cuda.empty_cache()

    res = {}
    # (device_direct / device_pinned: the fetch's two copy schemes, CCG_SNN_FETCH; device = the library's default)
    for name, emit, fetch in (("host", "host", None), ("device", "device", None), ("device_direct", "device", "direct"),
                              ("device_pinned", "device", "pinned")):
        os.environ.pop("CCG_SNN_FETCH", None)
        if fetch:
            os.environ["CCG_SNN_FETCH"] = fetch
        graphs = eng.snn_multi(kn, list(ks), "number", cell=boot_np, emit=emit)  # warm
        res[name] = graphs
        a, b, w = [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            graphs = eng.snn_multi(kn, list(ks), "number", cell=boot_np, emit=emit)
            w.append(1e3 * (time.perf_counter() - t0))
            a.append(1e3 * eng.last_snn_times[0])
            b.append(1e3 * eng.last_snn_times[1])
        first, second = ("pass", "decode") if emit == "host" else ("stage", "fetch")
        out[f"{name}_{first}_ms"] = med(a)
        out[f"{name}_{second}_ms"] = med(b)
        out[f"{name}_total_ms"] = med(w)
    os.environ.pop("CCG_SNN_FETCH", None)
    same = all(np.array_equal(x, y) for name in ("device", "device_direct", "device_pinned")
               for g, h in zip(res["host"], res[name]) for x, y in zip(g, h))
    assert same and [g[0].size for g in res["device"]] == edges
    out["lists_equal"] = bool(same)
    out["fetch_gb_per_s"] = out["fetch_bytes"] / out["device_fetch_ms"] / 1e6
    out["device_faster"] = bool(out["device_total_ms"] < out["host_total_ms"])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "snn_emit_micro.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
