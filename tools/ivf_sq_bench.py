#!/usr/bin/env python3
"""IVF_SQ beside IVF_FLAT (bound scan) and IVF_PQ (fp8 queries, m = 96), timed.

One handle per index type over the same rows: 1M x 768 f32, L2, clustered
synthetic data (1024 Gaussian clusters), nlist 1024, nprobe 32, B = 256, k = 10.
IVF_SQ is built by lance_detached_create_index; IVF_FLAT gets the same
centroids through lance_hip_ivf_set_model (the same lists are probed); IVF_PQ
trains its own model.  A fourth handle without an index gives the exact flat
search the recalls are measured against.

Per index type:
  * ms per synchronous lance_hip_search_batch_device call and queries / s:
    every leg warmed up, then --repeats windows of at least --window-s seconds
    of back-to-back calls, the legs alternating window by window in one
    process; median [min, max] of the windows;
  * the list-scan kernel's time per launch (option time_kernels: device events
    around the launch), its algorithmic bytes and their fraction of 8 TB/s;
  * recall@10 against the exact flat search at refine_factor 1, 2 and 4.

Before any timing the ids of an IVF_SQ search over a subsample (its own small
index) are checked against the numpy reference tests/sq_ref.py.

Writes one JSON document (--out, default profiles/ivf_sq.json) and prints it.
Needs a GPU: without a device it fails, it does not fall back."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "duckdb-lancedb_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--nlist", type=int, default=1024)
ap.add_argument("--nprobe", type=int, default=32)
ap.add_argument("--m", type=int, default=96)
ap.add_argument("--centers", type=int, default=1024)
ap.add_argument("--sigma", type=float, default=0.35)
ap.add_argument("--window-s", type=float, default=1.0)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--check-rows", type=int, default=20_000, help="rows of the sq_ref id check's own index")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_sq.json"))
a = ap.parse_args()

import lance_hip as hip  # noqa: E402  (imports torch first: one HIP runtime per process)
import torch  # noqa: E402

from oracle import flat_knn  # noqa: E402
from tests import sq_ref  # noqa: E402

L = hip.lib()
if hip.device_count() <= 0 or not torch.cuda.is_available():
    sys.exit("ivf_sq_bench: no HIP device (this tool measures on the GPU only)")
ERR = ctypes.create_string_buffer(2048)
HBM_BPS = 8e12


def say(*x):
    print("[ivf_sq_bench]", *x, file=sys.stderr, flush=True)


def chk(r, what):
    if r is None or (isinstance(r, int) and r < 0):
        sys.exit(f"ivf_sq_bench: {what}: {ERR.value.decode()}")
    return r


n, d, k, B = a.n, a.dim, a.k, a.batch
g = torch.Generator(device="cuda").manual_seed(1234)
Cc = torch.randn((a.centers, d), generator=g, device="cuda")
TYPES = ["ivf_sq", "ivf_flat", "ivf_pq"]
handles = {t: hip.LanceCreateDetached("", d, "l2", t) for t in TYPES + ["flat"]}
hip.LanceHipSetOption(handles["ivf_pq"], "pq_query", "fp8")
X0 = None
CH = 1 << 16
t0 = time.perf_counter()
for lo in range(0, n, CH):
    hi = min(n, lo + CH)
    lab = torch.randint(0, a.centers, (hi - lo,), generator=g, device="cuda")
    Xc = (Cc[lab] + a.sigma * torch.randn((hi - lo, d), generator=g, device="cuda")).cpu().numpy()
    if X0 is None:
        X0 = Xc[:a.check_rows].copy()
    for h in handles.values():
        hip.LanceDetachedAddBatch(h, Xc, hi - lo, d)
qi = torch.randint(0, a.centers, (B,), generator=g, device="cuda")
Qd = (Cc[qi] + a.sigma * torch.randn((B, d), generator=g, device="cuda")).contiguous()
Q = Qd.cpu().numpy()
say(f"rows loaded in {time.perf_counter() - t0:.1f} s")

# ---- ids against the numpy reference on a subsample (its own index) ---------------
hs = hip.LanceCreateDetached("", d, "l2", "check")
hip.LanceHipSetOption(hs, "index_type", "ivf_sq")
hip.LanceDetachedAddBatch(hs, X0, len(X0), d)
hip.LanceDetachedCreateIndex(hs, 32, 0)
ex = hip.LanceHipIvfExport(hs)
gl, gd, gc = hip.LanceDetachedSearchBatch(hs, Q[:16], k, nprobes=8, refine_factor=2)
el, ed, ec = sq_ref.ivf_sq_search(X0, ex["labels"], ex["live"], ex["lists"], ex["centroids"], ex["codebook"][0],
                                  ex["codebook"][1], Q[:16], k, 8, 2, "l2")
if not ((gc == ec).all() and (gl == el).all()):
    sys.exit("ivf_sq_bench: IVF_SQ ids differ from tests/sq_ref.py on the subsample")
hip.LanceFreeDetached(hs)
checked = {"rows": int(len(X0)), "queries": 16, "nlist": 32, "nprobe": 8, "refine": 2, "ids_match_sq_ref": True}
say("subsample ids match sq_ref")

# ---- indexes --------------------------------------------------------------------
build_s = {}
t0 = time.perf_counter()
hip.LanceHipSetOption(handles["ivf_sq"], "index_type", "ivf_sq")
hip.LanceDetachedCreateIndex(handles["ivf_sq"], a.nlist, 0)
build_s["ivf_sq"] = round(time.perf_counter() - t0, 2)
Cm = np.zeros((a.nlist, d), np.float32)
bounds = np.zeros(2, np.float32)
chk(L.lance_hip_ivf_export(handles["ivf_sq"], Cm.ctypes.data, bounds.ctypes.data, None, None, None, None, ERR, 2048),
    "ivf_export")
t0 = time.perf_counter()
hip.LanceHipIvfSetModel(handles["ivf_flat"], "ivf_flat", Cm)
build_s["ivf_flat (set_model)"] = round(time.perf_counter() - t0, 2)
t0 = time.perf_counter()
hip.LanceHipSetOption(handles["ivf_pq"], "index_type", "ivf_pq")
hip.LanceDetachedCreateIndex(handles["ivf_pq"], a.nlist, a.m)
build_s["ivf_pq"] = round(time.perf_counter() - t0, 2)
say("indexes built", build_s)

oL = torch.empty((B, k), dtype=torch.int64, device="cuda")
oD = torch.empty((B, k), dtype=torch.float32, device="cuda")
oC = torch.empty(B, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()


def step_of(h, refine):
    return lambda: chk(L.lance_hip_search_batch_device(h, Qd.data_ptr(), B, d, k, a.nprobe, refine, oL.data_ptr(),
                                                       oD.data_ptr(), oC.data_ptr(), ERR, 2048), "search")


# ---- recall against the exact flat search -----------------------------------------
step_of(handles["flat"], 1)()
torch.cuda.synchronize()
truth = oL.cpu().numpy().copy()
recall = {}
for t in TYPES:
    recall[t] = {}
    for rf in (1, 2, 4):
        step_of(handles[t], rf)()
        torch.cuda.synchronize()
        recall[t][f"refine_{rf}"] = round(float(flat_knn.recall_at_k(oL.cpu().numpy(), truth, k)), 4)
say("recall", recall)


# ---- timing ---------------------------------------------------------------------
def window(step):
    t0 = time.perf_counter()
    c = 0
    while True:
        step()
        c += 1
        if time.perf_counter() - t0 >= a.window_s:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / c, c


steps = {t: step_of(handles[t], 1) for t in TYPES}
for t in TYPES:
    t0 = time.perf_counter()
    c = 0
    while c < 5 or time.perf_counter() - t0 < 0.3:
        steps[t]()
        c += 1
res = {t: [] for t in TYPES}
for _ in range(a.repeats):
    for t in TYPES:
        ms, _ = window(steps[t])
        res[t].append(ms)
legs = {}
for t in TYPES:
    med = statistics.median(res[t])
    legs[t] = {"ms_per_call": round(med, 4), "min": round(min(res[t]), 4), "max": round(max(res[t]), 4),
               "windows": len(res[t]), "queries_per_s": round(B / med * 1e3, 1)}

# ---- list-scan kernel time (device events), in a pass of its own -----------------
for t in TYPES:
    h = handles[t]
    hip.LanceHipSetOption(h, "time_kernels", "1")
    steps[t]()
    k0 = hip.LanceHipKernelTimes(h)
    for _ in range(10):
        steps[t]()
    k1 = hip.LanceHipKernelTimes(h)
    hip.LanceHipSetOption(h, "time_kernels", "0")
    nl = k1["ivf_scan_launches"] - k0["ivf_scan_launches"]
    ms = (k1["ivf_scan_ms_total"] - k0["ivf_scan_ms_total"]) / max(nl, 1)
    by = (k1["ivf_scan_bytes"] - k0["ivf_scan_bytes"]) / max(nl, 1)
    pr = (k1["ivf_pair_rows"] - k0["ivf_pair_rows"]) / max(nl, 1)
    legs[t].update({"scan_kernel_ms": round(ms, 4), "scan_launches_timed": nl, "scan_algorithmic_bytes": by,
                    "scan_pair_rows": pr, "scan_fraction_of_8TBps": round(by / (ms * 1e-3) / HBM_BPS, 4) if ms > 0 else None})

info = {t: hip.LanceHipIvfInfo(handles[t]) for t in TYPES}
doc = {"tool": "tools/ivf_sq_bench.py", "device": torch.cuda.get_device_name(0), "library": hip.version(),
       "shape": {"n": n, "dim": d, "k": k, "batch": B, "metric": "l2", "storage": "f32", "nlist": a.nlist,
                 "nprobe": a.nprobe, "pq_m": a.m, "pq_query": "fp8",
                 "data": f"{a.centers} Gaussian clusters, centers N(0,1), sigma {a.sigma}; queries drawn the same way"},
       "sq_ref_check": checked, "sq_bounds": [float(bounds[0]), float(bounds[1])], "build_seconds": build_s,
       "window_s": a.window_s, "repeats": a.repeats,
       "timing": "host clock around synchronous lance_hip_search_batch_device calls (refine_factor 1), each window "
                 "ends in a device synchronise; median [min, max] of the windows; the legs alternate window by window "
                 "in one process; scan_kernel_ms: device events around the list-scan launch (time_kernels), 10 calls",
       "legs": legs, "recall_at_10_vs_exact_flat": recall, "ivf_info": info,
       "ratios": {"ivf_flat_over_ivf_sq_call": round(legs["ivf_flat"]["ms_per_call"] / legs["ivf_sq"]["ms_per_call"], 3),
                  "ivf_flat_over_ivf_sq_scan_kernel": round(legs["ivf_flat"]["scan_kernel_ms"] /
                                                            max(legs["ivf_sq"]["scan_kernel_ms"], 1e-9), 3),
                  "ivf_sq_over_ivf_flat_scan_bytes": round(legs["ivf_sq"]["scan_algorithmic_bytes"] /
                                                           max(legs["ivf_flat"]["scan_algorithmic_bytes"], 1.0), 3)}}
for h in handles.values():
    hip.LanceFreeDetached(h)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print(json.dumps(doc))
