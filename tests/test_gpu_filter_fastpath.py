"""GPU checks of filtered search as a first-class path: predicates evaluated on
the device (``csrc/filter_kernels.hip``), the per-handle filter cache, the int8
scan serving searches with a predicate, and the device-pointer entry point
``lance_hip_search_batch_device_filtered``.

Checkers: the host predicate evaluator (``lance_hip_predicate_mask``) for the
filters, the exact oracle restricted to numpy-computed masks for the searches.
Bar: labels bit-exact, distances within RTOL 1e-4 / ATOL 1e-5 (tests/test_gpu_filter.py).

Shapes: d = 128 is the smallest dimension the int8 copy accepts; n = 70_001 is
on the threshold path (> 65536 slots) with a ragged last tile and a partial last
ballot word; n = 3_000 is the dense path; n = 357 leaves most of the last
evaluator workgroup past the table."""
import ctypes

import numpy as np
import pyarrow as pa
import pytest

from oracle import c_oracle

pytestmark = pytest.mark.gpu

RTOL = 1e-4
ATOL = 1e-5


def assert_same(got, exp):
    (gl, gd, gc), (el, ed, ec) = got, exp
    np.testing.assert_array_equal(gc, ec)
    for i in range(el.shape[0]):
        n = int(gc[i])
        np.testing.assert_array_equal(gl[i, :n], el[i, :n], err_msg=f"query {i}")
        np.testing.assert_allclose(gd[i, :n], ed[i, :n], rtol=RTOL, atol=ATOL, err_msg=f"query {i}")


def _make(hip, X, extras, metric, options=()):
    batch = hip.arrow_rows(X, extras)
    with hip.ArrowC(batch) as sch:
        h = hip.LanceCreateDetachedFromArrow("", sch.schema_ptr, metric, "filt")
    for k, v in options:
        hip.LanceHipSetOption(h, k, v)
    with hip.ArrowC(batch) as a:
        labs = hip.LanceDetachedAddBatchArrow(h, a.schema_ptr, a.array_ptr)
    assert labs.tolist() == list(range(len(X)))
    return h


def _append(hip, h, X, extras):
    with hip.ArrowC(hip.arrow_rows(X, extras)) as a:
        return hip.LanceDetachedAddBatchArrow(h, a.schema_ptr, a.array_ptr)


def _info(hip, h):
    return hip.LanceHipFilterInfo(h)


# ---------------------------------------------------------------------------
# evaluator kernel
# ---------------------------------------------------------------------------
NUMERIC_PREDS = [
    "i32 < 10", "7 >= i32", "i64 = 2000000000000", "i64 != 4611686018427387905", "i64 > 4.0e18", "f64 > 0.5",
    "f64 >= f64", "f64 IS NULL", "f64 IS NOT NULL", "flag", "NOT flag", "flag = false",
    "i32 IN (1, 2, 3, NULL)", "i32 NOT IN (5, 7)", "f64 BETWEEN -1 AND 1", "i32 NOT BETWEEN -5 AND 5", "i32 < i64",
    "NOT (NOT (i32 < 0 OR f64 > 1))", "(i32 < 0 AND flag) OR (f64 IS NULL AND NOT (i64 > 0))", "(f64 < 0) IS NULL",
    "label >= 37 AND label < 101", "label BETWEEN 65 AND 127", "label > 60 AND label <= 70000 AND NOT (label = 320)",
    "label IN (0, 63, 64, 65, 356, 70000)", "true", "NULL",
]
STRING_PREDS = ["lang = 'en'", "lang IS NULL OR i32 > 3"]


def _eval_table(rng, n):
    def arr(vals, typ, p):
        return pa.array(vals, typ, mask=rng.random(n) < p)

    f = rng.normal(0, 2, n)
    f[rng.random(n) < 0.05] = np.nan
    big = np.where(rng.random(n) < 0.1, (1 << 62) + rng.integers(0, 3, n), rng.integers(-3, 3, n) * 10**12)
    langs = np.array(["en", "fr", "de"], object)
    return [("i32", arr(rng.integers(-20, 20, n).astype(np.int32), pa.int32(), 0.1), None),
            ("i64", arr(big.astype(np.int64), pa.int64(), 0.1), None),
            ("f64", arr(f, pa.float64(), 0.1), None),
            ("flag", arr(rng.random(n) < 0.5, pa.bool_(), 0.1), None),
            ("lang", arr(langs[rng.integers(0, 3, n)], pa.string(), 0.1), None)]


@pytest.mark.parametrize("n", [357, 70_001])
def test_device_evaluator_matches_host_evaluator(hip, n):
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, 8)).astype(np.float32)
    extras = _eval_table(rng, n)
    batch = hip.arrow_rows(X, extras)
    dead = rng.choice(n, n // 20, replace=False)
    live = np.ones(n, np.uint8)
    live[dead] = 0
    labels = np.arange(n)
    h = _make(hip, X, extras, "l2")
    hh = _make(hip, X, extras, "l2", options=[("filter_eval", "host")])
    try:
        for x in (h, hh):
            hip.LanceDetachedDeleteBatch(x, dead)
        for preds, dev in ((NUMERIC_PREDS, True), (STRING_PREDS, False)):
            for pred in preds:
                exp = hip.LanceHipPredicateMask(batch, labels, live, pred)
                before, hbefore = _info(hip, h), _info(hip, hh)
                got = hip.LanceHipFilterMask(h, pred)
                assert got.shape == (n,) and got.tobytes() == exp.tobytes(), pred
                after = _info(hip, h)
                assert after["device_evals"] - before["device_evals"] == (1 if dev else 0), pred
                assert after["host_evals"] - before["host_evals"] == (0 if dev else 1), pred
                assert after["last_selected"] == int(exp.sum()), pred
                # filter_eval = host: the same filter, the host evaluator only
                assert hip.LanceHipFilterMask(hh, pred).tobytes() == exp.tobytes(), pred
                hafter = _info(hip, hh)
                assert hafter["device_evals"] == 0 and hafter["host_evals"] == hbefore["host_evals"] + 1, pred
        with pytest.raises(hip.IOException, match="output buffer too small"):
            hip.LanceHipFilterMask(h, "flag", capacity=n - 1)
        with pytest.raises(hip.IOException, match="no column named 'nosuch'"):
            hip.LanceHipFilterMask(h, "nosuch = 1")
        with pytest.raises(hip.IOException, match="predicate: "):
            hip.LanceHipFilterPrepare(h, "i32 = ")
    finally:
        hip.LanceFreeDetached(h)
        hip.LanceFreeDetached(hh)


# ---------------------------------------------------------------------------
# the int8 scan serves predicates
# ---------------------------------------------------------------------------
D8 = 128


def _search_table(rng, n):
    """sel uniform in [0, 1000); tag = 1 on exactly 7 rows, 0 elsewhere."""
    sel = rng.integers(0, 1000, n)
    tag = np.zeros(n, np.int32)
    tag[rng.choice(n, 7, replace=False)] = 1
    return sel, tag


def _extras(sel, tag):
    return [("sel", pa.array(sel, pa.int64()), None), ("tag", pa.array(tag, pa.int32()), None)]


@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
@pytest.mark.parametrize("n", [3_000, 70_001])
def test_int8_scan_serves_filtered_search(hip, metric, n):
    rng = np.random.default_rng(n + len(metric))
    X = rng.standard_normal((n, D8)).astype(np.float32)
    Q = rng.standard_normal((40, D8)).astype(np.float32)
    sel, tag = _search_table(rng, n)
    dead = rng.choice(np.flatnonzero(tag == 0), n // 20, replace=False)
    live = np.ones(n, bool)
    live[dead] = False
    h = _make(hip, X, _extras(sel, tag), metric, options=[("time_kernels", "1")])
    h16 = _make(hip, X, _extras(sel, tag), metric, options=[("scan_i8", "off")])
    try:
        for x in (h, h16):
            hip.LanceDetachedDeleteBatch(x, dead)
        cases = [("sel < 500", live & (sel < 500)), ("sel < 100", live & (sel < 100)), ("tag = 1", live & (tag == 1)),
                 ("tag = 2", np.zeros(n, bool))]
        assert int(cases[2][1].sum()) == 7
        kernels = set()
        for pred, m in cases:
            for k in ([10, 40] if n > 65536 else [10]):
                exp = c_oracle.flat_search_batch(X, Q, k, metric, live=m, acc64=True, nthreads=16)
                got = hip.LanceDetachedSearchBatch(h, Q, k, predicate=pred)
                assert_same(got, exp)
                if m.any():
                    kt = hip.LanceHipKernelTimes(h)
                    assert kt["scan_elem_bytes"] == 1, (pred, k, kt)  # the int8 copy was streamed
                    kernels.add(kt["scan_kernel"])
                else:
                    assert (got[2] == 0).all() and (got[0] == -1).all()
                ref = hip.LanceDetachedSearchBatch(h16, Q, k, predicate=pred)
                np.testing.assert_array_equal(got[2], ref[2])
                for i in range(len(Q)):
                    np.testing.assert_array_equal(got[0][i, :got[2][i]], ref[0][i, :ref[2][i]])
        assert hip.LanceHipKernelTimes(h16)["scan_elem_bytes"] == 2
        # an unfiltered search afterwards is unchanged
        exp = c_oracle.flat_search_batch(X, Q, 10, metric, live=live, acc64=True, nthreads=16)
        assert_same(hip.LanceDetachedSearchBatch(h, Q, 10), exp)
        kt = hip.LanceHipKernelTimes(h)
        assert kt["scan_elem_bytes"] == 1
        # (at d = 128 the int8 rows go through scan_kernel: scan8_kernel takes rows of >= 512 elements,
        # test_int8_threshold_kernel_serves_filtered_search); with or without a predicate, the same kernel
        assert kernels == {kt["scan_kernel"]}
    finally:
        hip.LanceFreeDetached(h)
        hip.LanceFreeDetached(h16)


def test_int8_threshold_kernel_serves_filtered_search(hip):
    # d = 512 is the smallest row scan8_kernel (the int8 threshold kernel) takes
    rng = np.random.default_rng(512)
    n, d, k = 70_001, 512, 10
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((40, d)).astype(np.float32)
    sel, tag = _search_table(rng, n)
    h = _make(hip, X, _extras(sel, tag), "l2", options=[("time_kernels", "1")])
    try:
        for pred, m in [("sel < 500", sel < 500), ("sel < 100", sel < 100)]:
            exp = c_oracle.flat_search_batch(X, Q, k, "l2", live=m, acc64=True, nthreads=16)
            n0 = hip.LanceHipKernelTimes(h)["scan_launches"]
            assert_same(hip.LanceDetachedSearchBatch(h, Q, k, predicate=pred), exp)
            kt = hip.LanceHipKernelTimes(h)
            assert kt["scan_launches"] > n0 and kt["scan_rows"] == n, kt  # this search's threshold scan was timed
            assert kt["scan_elem_bytes"] == 1 and kt["scan_kernel"] == "scan8_kernel", kt
    finally:
        hip.LanceFreeDetached(h)


# ---------------------------------------------------------------------------
# cache and staleness
# ---------------------------------------------------------------------------
def test_filter_cache_and_staleness(hip):
    rng = np.random.default_rng(77)
    n, k = 70_001, 10
    X = rng.standard_normal((n, D8)).astype(np.float32)
    Q = rng.standard_normal((40, D8)).astype(np.float32)
    score = rng.integers(0, 1000, n)
    pred = "score < 500"

    def extras(s):
        return [("score", pa.array(s, pa.int64()), None)]

    def oracle(Xa, m):
        return c_oracle.flat_search_batch(Xa, Q, k, "l2", live=m, acc64=True, nthreads=16)

    h = _make(hip, X, extras(score), "l2")
    try:
        live = np.ones(n, bool)
        exp = oracle(X, live & (score < 500))
        i0 = _info(hip, h)
        assert_same(hip.LanceDetachedSearchBatch(h, Q, k, predicate=pred), exp)
        i1 = _info(hip, h)
        assert (i1["misses"] - i0["misses"], i1["hits"] - i0["hits"]) == (1, 0)
        assert i1["device_evals"] == 1 and i1["masked_copies"] > i0["masked_copies"]
        assert_same(hip.LanceDetachedSearchBatch(h, Q, k, predicate=pred), exp)
        i2 = _info(hip, h)
        assert (i2["misses"] - i1["misses"], i2["hits"] - i1["hits"]) == (0, 1)
        assert i2["masked_copies"] == i1["masked_copies"]  # the masked row terms were reused too

        # delete the top-1 of query 0: the cached filter is stale
        top = int(exp[0][0, 0])
        hip.LanceDetachedDelete(h, top)
        live[top] = False
        exp = oracle(X, live & (score < 500))
        got = hip.LanceDetachedSearchBatch(h, Q, k, predicate=pred)
        i3 = _info(hip, h)
        assert (i3["misses"] - i2["misses"], i3["hits"] - i2["hits"]) == (1, 0)
        assert top not in got[0][0].tolist()
        assert_same(got, exp)

        # append copies of queries with matching metadata: a miss, and they are the top-1
        labs = _append(hip, h, Q[:10], extras(np.zeros(10, np.int64)))
        assert labs.tolist() == list(range(n, n + 10))
        got = hip.LanceDetachedSearchBatch(h, Q, k, predicate=pred)
        i4 = _info(hip, h)
        assert (i4["misses"] - i3["misses"], i4["hits"] - i3["hits"]) == (1, 0)
        assert got[0][:10, 0].tolist() == list(range(n, n + 10))
        # ... and with non-matching metadata: never returned
        _append(hip, h, Q[10:20], extras(np.full(10, 900, np.int64)))
        Xa = np.concatenate([X, Q[:20]])
        sa = np.concatenate([score, np.zeros(10, np.int64), np.full(10, 900, np.int64)])
        la = np.concatenate([live, np.ones(20, bool)])
        preds = {pred: la & (sa < 500), "score >= 900": la & (sa >= 900), "score BETWEEN 100 AND 199": la & (sa >= 100) & (sa <= 199)}
        exps = {p: oracle(Xa, m) for p, m in preds.items()}
        got = hip.LanceDetachedSearchBatch(h, Q, k, predicate=pred)
        assert not (got[0] >= n + 10).any()
        assert_same(got, exps[pred])

        hip.LanceDetachedCompact(h)  # labels stay, slots move: a miss, the same results
        i5 = _info(hip, h)
        assert_same(hip.LanceDetachedSearchBatch(h, Q, k, predicate=pred), exps[pred])
        i6 = _info(hip, h)
        assert (i6["misses"] - i5["misses"], i6["hits"] - i5["hits"]) == (1, 0)

        # two predicates alternating within the capacity: hits only after their first use
        two = [pred, "score >= 900"]
        assert_same(hip.LanceDetachedSearchBatch(h, Q, k, predicate=two[1]), exps[two[1]])
        i7 = _info(hip, h)
        for r in range(4):
            assert_same(hip.LanceDetachedSearchBatch(h, Q, k, predicate=two[r % 2]), exps[two[r % 2]])
        i8 = _info(hip, h)
        assert (i8["misses"] - i7["misses"], i8["hits"] - i7["hits"]) == (0, 4)

        # three predicates in rotation through a cache of two: still exact
        hip.LanceHipSetOption(h, "filter_cache", "2")
        assert _info(hip, h)["entries"] == 2
        for r in range(6):
            p = list(preds)[r % 3]
            assert_same(hip.LanceDetachedSearchBatch(h, Q, k, predicate=p), exps[p])
        assert _info(hip, h)["entries"] == 2

        # no cache: every call evaluates, still exact
        hip.LanceHipSetOption(h, "filter_cache", "0")
        i9 = _info(hip, h)
        assert i9["entries"] == 0
        for r in range(3):
            assert_same(hip.LanceDetachedSearchBatch(h, Q, k, predicate=pred), exps[pred])
        i10 = _info(hip, h)
        assert (i10["misses"] - i9["misses"], i10["hits"] - i9["hits"]) == (3, 0)

        # prepare: the oracle's count now, a hit at the search that follows
        hip.LanceHipSetOption(h, "filter_cache", "8")
        p = "score BETWEEN 100 AND 199"
        assert hip.LanceHipFilterPrepare(h, p) == int(preds[p].sum())
        i11 = _info(hip, h)
        assert i11["last_selected"] == int(preds[p].sum())
        assert_same(hip.LanceDetachedSearchBatch(h, Q, k, predicate=p), exps[p])
        i12 = _info(hip, h)
        assert (i12["misses"] - i11["misses"], i12["hits"] - i11["hits"]) == (0, 1)
    finally:
        hip.LanceFreeDetached(h)


# ---------------------------------------------------------------------------
# device-pointer entry point
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("index_type", [None, "ivf_flat"])
def test_device_pointer_filtered_search(hip, index_type):
    import torch

    rng = np.random.default_rng(21)
    n, d, nlist, k = 20_000, 32, 40, 10
    C = rng.standard_normal((30, d)).astype(np.float32)
    X = (C[rng.integers(0, 30, n)] + 0.4 * rng.standard_normal((n, d))).astype(np.float32)
    Q = (X[rng.choice(n, 30, replace=False)] + 0.1 * rng.standard_normal((30, d))).astype(np.float32)
    score = rng.integers(0, 1000, n)
    lang = np.array(["en", "fr", "es"], object)[rng.integers(0, 3, n)]
    h = _make(hip, X, [("score", pa.array(score, pa.int64()), None), ("lang", pa.array(lang, pa.string()), None)], "l2")
    try:
        if index_type:
            sel = hip.LanceHipFilterPrepare(h, "score < 300")
            assert sel == int((score < 300).sum())
            hip.LanceHipSetOption(h, "index_type", index_type)
            hip.LanceDetachedCreateIndex(h, nlist, 8)
            # create_index: the filter cached before it is stale
            i0 = _info(hip, h)
            assert hip.LanceHipFilterPrepare(h, "score < 300") == sel
            i1 = _info(hip, h)
            assert (i1["misses"] - i0["misses"], i1["hits"] - i0["hits"]) == (1, 0)
        Qd = torch.from_numpy(Q).cuda()
        for pred in ["score < 300", "lang = 'en' AND score >= 100", "score > 5000"]:
            el, ed, ec = hip.LanceDetachedSearchBatch(h, Q, k, nprobes=6, refine_factor=3, predicate=pred)
            gl, gd, gc = hip.LanceHipSearchBatchDeviceFiltered(h, Qd, k, nprobes=6, refine_factor=3, predicate=pred)
            gl, gd, gc = gl.cpu().numpy(), gd.cpu().numpy(), gc.cpu().numpy()
            np.testing.assert_array_equal(gc, ec)
            assert (ec > 0).all() or pred == "score > 5000"
            for i in range(len(Q)):
                np.testing.assert_array_equal(gl[i, :gc[i]], el[i, :ec[i]])
                np.testing.assert_array_equal(gd[i, :gc[i]], ed[i, :ec[i]])
            if pred == "score > 5000":  # no selected row: the host API's fill
                assert (gc == 0).all() and (gl == -1).all() and np.isnan(gd).all()
        # a NULL or empty predicate is lance_hip_search_batch_device
        L = hip.lib()
        ol = torch.empty((len(Q), k), dtype=torch.int64, device="cuda")
        od = torch.empty((len(Q), k), dtype=torch.float32, device="cuda")
        oc = torch.empty(len(Q), dtype=torch.int32, device="cuda")
        e = ctypes.create_string_buffer(2048)
        torch.cuda.synchronize()
        assert L.lance_hip_search_batch_device(h, Qd.data_ptr(), len(Q), d, k, 6, 3, ol.data_ptr(), od.data_ptr(),
                                               oc.data_ptr(), e, 2048) == len(Q), e.value
        el, ed, ec = ol.cpu().numpy(), od.cpu().numpy(), oc.cpu().numpy()
        assert (ec > 0).all()
        for p in (None, ""):
            gl, gd, gc = hip.LanceHipSearchBatchDeviceFiltered(h, Qd, k, nprobes=6, refine_factor=3, predicate=p)
            gl, gd, gc = gl.cpu().numpy(), gd.cpu().numpy(), gc.cpu().numpy()
            np.testing.assert_array_equal(gc, ec)
            for i in range(len(Q)):
                np.testing.assert_array_equal(gl[i, :gc[i]], el[i, :ec[i]])
                np.testing.assert_array_equal(gd[i, :gc[i]], ed[i, :ec[i]])
        before = hip.LanceHipFilterInfo(h)
        with pytest.raises(hip.IOException, match="no column named 'nosuch'"):
            hip.LanceHipSearchBatchDeviceFiltered(h, Qd, k, predicate="nosuch = 1")
        with pytest.raises(hip.IOException, match="predicate: "):
            hip.LanceHipSearchBatchDeviceFiltered(h, Qd, k, predicate="score < ")
        assert hip.LanceHipFilterInfo(h)["entries"] == before["entries"]
    finally:
        hip.LanceFreeDetached(h)


def test_device_pointer_filtered_search_on_a_two_shard_handle(hip):
    # both shards on device 0 (runs on every box): the predicate's filter per shard, the merge on the device
    import torch

    rng = np.random.default_rng(33)
    n, d, k = 20_000, 32, 10
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((30, d)).astype(np.float32)
    h = hip.LanceCreateDetached("", d, "l2", "t")
    try:
        hip.LanceHipSetOption(h, "devices", "0,0")
        for lo in range(0, n, 5000):
            hip.LanceDetachedAddBatch(h, X[lo:lo + 5000], 5000, d)
        dead = rng.choice(n, 500, replace=False)
        hip.LanceDetachedDeleteBatch(h, dead)
        labels = np.arange(n)
        m = (labels < 4000) | (labels >= 13_000)
        m[dead] = False
        pred = "label < 4000 OR label >= 13000"
        exp = c_oracle.flat_search_batch(X, Q, k, "l2", live=m, acc64=True, nthreads=16)
        assert hip.LanceHipFilterPrepare(h, pred) == int(m.sum())
        host = hip.LanceDetachedSearchBatch(h, Q, k, predicate=pred)
        assert_same(host, exp)
        gl, gd, gc = hip.LanceHipSearchBatchDeviceFiltered(h, torch.from_numpy(Q).cuda(), k, predicate=pred)
        gl, gd, gc = gl.cpu().numpy(), gd.cpu().numpy(), gc.cpu().numpy()
        np.testing.assert_array_equal(gc, host[2])
        np.testing.assert_array_equal(gl, host[0])
        np.testing.assert_array_equal(gd, host[1])
        info = _info(hip, h)  # the first store's counters: one evaluation, then hits
        assert info["misses"] == 1 and info["hits"] == 2 and info["device_evals"] == 1, info
        with pytest.raises(hip.IOException, match="multi-device"):
            hip.LanceHipFilterMask(h, pred)
    finally:
        hip.LanceFreeDetached(h)


# ---------------------------------------------------------------------------
# one query per call
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3_000, 70_001])
def test_one_query_per_call_with_predicate(hip, n):
    rng = np.random.default_rng(n + 1)
    X = rng.standard_normal((n, D8)).astype(np.float32)
    Q = rng.standard_normal((4, D8)).astype(np.float32)
    sel, tag = _search_table(rng, n)
    pred, k = "sel < 250", 10
    h = _make(hip, X, _extras(sel, tag), "l2")
    try:
        exp = c_oracle.flat_search_batch(X, Q, k, "l2", live=sel < 250, acc64=True, nthreads=16)
        batch = hip.LanceDetachedSearchBatch(h, Q, k, predicate=pred)
        assert_same(batch, exp)
        i0 = _info(hip, h)
        for rep in range(3):
            for i in range(len(Q)):
                lab, dist = hip.LanceDetachedSearch(h, Q[i], D8, k, predicate=pred)
                np.testing.assert_array_equal(lab, batch[0][i, :batch[2][i]])
                np.testing.assert_allclose(dist, batch[1][i, :batch[2][i]], rtol=RTOL, atol=ATOL)
        i1 = _info(hip, h)
        assert (i1["misses"] - i0["misses"], i1["hits"] - i0["hits"]) == (0, 3 * len(Q))
        if n <= 32768:
            assert hip.LanceHipLastSearchStats(h)["small_exact"]
    finally:
        hip.LanceFreeDetached(h)
