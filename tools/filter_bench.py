#!/usr/bin/env python3
"""Filtered search on the C2 shape (1M x 768 f32, L2, k = 10), timed.

Table: the C2 rows plus an int64 column `bucket` uniform in [0, 100) and a
string column `cat` ("c0" .. "c9").  Predicates: `bucket < 10`, `bucket < 50`
(device-evaluated) and `cat = 'c3'` (the host-route case).

Legs (every leg: warmed up, then --repeats windows of at least --window-s
seconds of back-to-back calls; every call is synchronous, the window ends in a
device synchronise; reported: median, min and max of the windows' ms per call):
  * batched B = 256 through lance_hip_search_batch_device_filtered, the
    predicate repeated (filter-cache hit) and with filter_cache = 0 (every call
    evaluates), beside the unfiltered synchronous lance_hip_search_batch_device;
  * one query per call through lance_detached_search_with_predicate, both ways;
  * the host-pointer batch lance_detached_search_batch with the predicate.
With --parent-lib (the parent commit's liblancedb_hip.so built to a second
path, e.g. `make -C duckdb-lancedb_amd` in a checkout of that commit and its
lib/liblancedb_hip.so copied to duckdb-lancedb_amd/lib_dev/, which git ignores,
as tools/devlib.sh's variants are) the legs the parent can run (host-pointer
batch, per call) are timed on it too, old and new alternating window by window
over the same rows.

Before any timing the ids of the filtered searches are checked once against the
CPU oracle's prefilter (oracle/flat_knn.c over the selected rows).

Writes one JSON document (--out, default profiles/filter_fastpath.json) and
prints it.  Needs a GPU: without a device it fails, it does not fall back."""
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
ap.add_argument("--window-s", type=float, default=1.0)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--check-queries", type=int, default=32, help="queries of the oracle id check")
ap.add_argument("--parent-lib", default=None, help="the parent commit's liblancedb_hip.so (A/B legs)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_fastpath.json"))
ap.add_argument("--profile-steps", type=int, default=0,
                help="only run this many cache-hit `bucket < 10` batched steps after the warm-up (for a "
                     "rocprofv3 --kernel-trace --stats run of its own) and exit")
a = ap.parse_args()

import lance_hip  # noqa: E402  (imports torch first: one HIP runtime per process)
import pyarrow as pa  # noqa: E402
import torch  # noqa: E402

from oracle import c_oracle  # noqa: E402

NEW = lance_hip.lib()
if lance_hip.device_count() <= 0 or not torch.cuda.is_available():
    sys.exit("filter_bench: no HIP device (this tool measures on the GPU only)")


def bind(path):
    L = ctypes.CDLL(path)
    for name, res, args in lance_hip._SIGNATURES:
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
    return L


OLD = bind(a.parent_lib) if a.parent_lib else None
ERR = ctypes.create_string_buffer(2048)


def chk(r, what):
    if r is None or (isinstance(r, int) and r < 0):
        sys.exit(f"filter_bench: {what}: {ERR.value.decode()}")
    return r


PREDS = ["bucket < 10", "bucket < 50", "cat = 'c3'"]
rng = np.random.default_rng(1234)
n, d, k, B = a.n, a.dim, a.k, a.batch
bucket = rng.integers(0, 100, n)
cat = rng.integers(0, 10, n)
cat_s = np.array([f"c{i}" for i in range(10)], object)[cat]
MASKS = {"bucket < 10": bucket < 10, "bucket < 50": bucket < 50, "cat = 'c3'": cat == 3}
X = np.empty((n, d), np.float32)
Q = rng.standard_normal((B, d), dtype=np.float32)
libs = [("new", NEW)] + ([("parent", OLD)] if OLD else [])
handles = {}
CH = 1 << 16
for lo in range(0, n, CH):
    hi = min(n, lo + CH)
    X[lo:hi] = rng.standard_normal((hi - lo, d), dtype=np.float32)
    batch = lance_hip.arrow_rows(X[lo:hi], [("bucket", pa.array(bucket[lo:hi], pa.int64()), None),
                                            ("cat", pa.array(cat_s[lo:hi], pa.string()), None)])
    for name, L in libs:
        if name not in handles:
            with lance_hip.ArrowC(batch) as s:
                handles[name] = chk(L.lance_create_detached_from_arrow(b"", s.schema_ptr, b"l2", b"fb", ERR, 2048), "create")
        with lance_hip.ArrowC(batch) as s:
            out = np.empty(hi - lo, np.int64)
            chk(L.lance_detached_add_batch_arrow(handles[name], s.schema_ptr, s.array_ptr, out.ctypes.data, ERR, 2048), "add")
for name, L in libs:
    chk(L.lance_hip_set_option(handles[name], b"prepare", b"1", ERR, 2048), "prepare")

Qd = torch.from_numpy(Q).cuda()
oL = torch.empty((B, k), dtype=torch.int64, device="cuda")
oD = torch.empty((B, k), dtype=torch.float32, device="cuda")
oC = torch.empty(B, dtype=torch.int32, device="cuda")
hL, hD, hC = np.empty((B, k), np.int64), np.empty((B, k), np.float32), np.empty(B, np.int32)
torch.cuda.synchronize()


def dev_step(L, h, pred):
    p = None if pred is None else pred.encode()
    if p is None:
        return lambda: chk(L.lance_hip_search_batch_device(h, Qd.data_ptr(), B, d, k, 20, 1, oL.data_ptr(), oD.data_ptr(),
                                                           oC.data_ptr(), ERR, 2048), "search")
    return lambda: chk(L.lance_hip_search_batch_device_filtered(h, Qd.data_ptr(), B, d, k, 20, 1, p, oL.data_ptr(),
                                                                oD.data_ptr(), oC.data_ptr(), ERR, 2048), "search")


def host_step(L, h, pred):
    p = pred.encode()
    return lambda: chk(L.lance_detached_search_batch(h, Q.ctypes.data, B, d, k, 20, 1, p, hL.ctypes.data, hD.ctypes.data,
                                                     hC.ctypes.data, ERR, 2048), "search")


def percall_step(L, h, pred):
    p = pred.encode()
    state = {"i": 0}

    def step():
        i = state["i"] = (state["i"] + 1) % B
        chk(L.lance_detached_search_with_predicate(h, Q[i].ctypes.data, d, k, 20, 1, p, hL.ctypes.data, hD.ctypes.data,
                                                   ERR, 2048), "search")
    return step


def cache(L, h, cap):
    return lambda: chk(L.lance_hip_set_option(h, b"filter_cache", str(cap).encode(), ERR, 2048), "set_option")


# ---- ids against the oracle's prefilter, once ---------------------------------
cq = min(a.check_queries, B)
checked = {}
for pred in PREDS:
    el, ed, ec = c_oracle.flat_search_batch(X, Q[:cq], k, "l2", live=MASKS[pred], acc64=True, nthreads=16)
    dev_step(NEW, handles["new"], pred)()
    gl, gc = oL.cpu().numpy(), oC.cpu().numpy()
    for name, L in libs:
        host_step(L, handles[name], pred)()
        if not ((hC[:cq] == ec).all() and (hL[:cq] == el).all()):
            sys.exit(f"filter_bench: {name} library's ids differ from the oracle's for {pred!r}")
    if not ((gc[:cq] == ec).all() and (gl[:cq] == el).all() and (gl == hL).all()):
        sys.exit(f"filter_bench: device-pointer ids differ from the oracle's for {pred!r}")
    checked[pred] = {"queries": cq, "selected": int(MASKS[pred].sum()), "ids_match_oracle": True}

if a.profile_steps:
    step = dev_step(NEW, handles["new"], PREDS[0])
    for _ in range(50 + a.profile_steps):
        step()
    torch.cuda.synchronize()
    sys.exit(0)


# ---- timing --------------------------------------------------------------------
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


def measure(group):
    """group: [(leg name, setup or None, step)]; the legs alternate window by window."""
    res = {nm: [] for nm, _, _ in group}
    calls = {}
    for nm, setup, step in group:  # warm up every shape
        if setup:
            setup()
        t0 = time.perf_counter()
        c = 0
        while c < 5 or time.perf_counter() - t0 < 0.3:
            step()
            c += 1
    for _ in range(a.repeats):
        for nm, setup, step in group:
            if setup:
                setup()
                step()  # (untimed: the first call after an option change re-evaluates)
            ms, c = window(step)
            res[nm].append(ms)
            calls[nm] = c
    return {nm: {"ms_per_call": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5),
                 "windows": len(v), "calls_last_window": calls[nm]} for nm, v in res.items()}


hn = handles["new"]
legs = {}
legs.update(measure([("batched_unfiltered_sync", None, dev_step(NEW, hn, None))]))
for pred in PREDS:
    legs.update(measure([(f"batched_hit[{pred}]", cache(NEW, hn, 8), dev_step(NEW, hn, pred)),
                         (f"batched_miss[{pred}]", cache(NEW, hn, 0), dev_step(NEW, hn, pred))]))
cache(NEW, hn, 8)()
for pred in PREDS[:2]:
    g = [(f"percall_hit[{pred}]", cache(NEW, hn, 8), percall_step(NEW, hn, pred)),
         (f"percall_miss[{pred}]", cache(NEW, hn, 0), percall_step(NEW, hn, pred))]
    if OLD:
        g.append((f"parent_percall[{pred}]", None, percall_step(OLD, handles["parent"], pred)))
    legs.update(measure(g))
    cache(NEW, hn, 8)()
    g = [(f"hostbatch[{pred}]", None, host_step(NEW, hn, pred))]
    if OLD:
        g.append((f"parent_hostbatch[{pred}]", None, host_step(OLD, handles["parent"], pred)))
    legs.update(measure(g))

info = lance_hip.LanceHipFilterInfo(hn)
ms = {nm: v["ms_per_call"] for nm, v in legs.items()}
ratios = {}
for pred in PREDS:
    ratios[f"filtered_over_unfiltered[{pred}]"] = round(ms[f"batched_hit[{pred}]"] / ms["batched_unfiltered_sync"], 3)
    ratios[f"miss_over_hit_batched[{pred}]"] = round(ms[f"batched_miss[{pred}]"] / ms[f"batched_hit[{pred}]"], 3)
for pred in PREDS[:2]:
    ratios[f"miss_over_hit_percall[{pred}]"] = round(ms[f"percall_miss[{pred}]"] / ms[f"percall_hit[{pred}]"], 3)
    if OLD:
        for leg, new in (("percall", f"percall_hit[{pred}]"), ("hostbatch", f"hostbatch[{pred}]")):
            old = legs[f"parent_{leg}[{pred}]"]
            ratios[f"parent_over_new_{leg}[{pred}]"] = round(old["ms_per_call"] / ms[new], 3)
            # faster by more than the repeat-to-repeat spread: the windows do not overlap
            ratios[f"new_faster_beyond_spread_{leg}[{pred}]"] = bool(legs[new]["max"] < old["min"])
targets = {"percall_ms_target": 0.30, "batched_within_of_unfiltered_target": 1.3,
           "percall_ms": {p: ms[f"percall_hit[{p}]"] for p in PREDS[:2]},
           "batched_ratio": {p: ratios[f"filtered_over_unfiltered[{p}]"] for p in PREDS}}
doc = {"tool": "tools/filter_bench.py", "device": torch.cuda.get_device_name(0), "library": lance_hip.version(),
       "shape": {"n": n, "dim": d, "k": k, "batch": B, "metric": "l2", "storage": "f32"},
       "predicates": checked, "window_s": a.window_s, "repeats": a.repeats,
       "timing": "host clock around synchronous calls, each window ends in a device synchronise; median [min, max] "
                 "of the windows; parent and new legs alternate window by window in one process",
       "parent_lib": bool(OLD), "legs": legs, "ratios": ratios, "targets": targets, "filter_info": info}
for name, L in libs:
    L.lance_free_detached(handles[name])
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print(json.dumps(doc))
