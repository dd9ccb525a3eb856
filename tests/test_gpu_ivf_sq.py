"""GPU parity of the IVF_SQ index (index_type = ivf_sq, and what
lance_detached_create_hnsw_index builds: rust_lib/src/lance_manager.rs:517-551,
IvfHnswSqIndexBuilder, without the per-partition graph) against the numpy
reference tests/sq_ref.py, given the model and lists the library exports.
Bar: labels bit-exact, distances within 1e-4 relative / 1e-5 absolute (the bar
of test_gpu_ivf.py)."""
import numpy as np
import pytest

from oracle import flat_knn
from tests import sq_ref
from tests.golden_runner import hnsw_rows
from tests.test_gpu_bf16 import bf16_round

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


@pytest.fixture
def mk(hip):
    made = []

    def make(dim, metric="l2", path="", storage=None, table="ivfsq", options=()):
        h = hip.LanceCreateDetached(path, dim, metric, table)
        made.append(h)
        if storage:
            hip.LanceHipSetOption(h, "storage", storage)
        hip.LanceHipSetOption(h, "index_type", "ivf_sq")
        for k, v in options:
            hip.LanceHipSetOption(h, k, v)
        return h

    yield make
    for h in made:
        hip.LanceFreeDetached(h)


def clustered(rng, n, d, centers=48, spread=0.35):
    C = rng.standard_normal((centers, d)).astype(np.float32)
    lab = rng.integers(0, centers, n)
    return (C[lab] + spread * rng.standard_normal((n, d))).astype(np.float32)


def ref_search(hip, h, X_by_label, Q, k, nprobe, rf, metric, tie=None, selected=None):
    ex = hip.LanceHipIvfExport(h)
    assert ex["type"] == "ivf_sq"
    X = X_by_label[ex["labels"]]
    live = ex["live"] if selected is None else ex["live"] & selected[ex["labels"]]
    lo, hi = ex["codebook"]
    return sq_ref.ivf_sq_search(X, ex["labels"], live, ex["lists"], ex["centroids"], lo, hi, Q, k, nprobe, rf, metric,
                                tie=tie)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(1)
    n, d = 3000, 128
    X = clustered(rng, n, d)
    Q = (X[rng.choice(n, 40, replace=False)] + 0.2 * rng.standard_normal((40, d))).astype(np.float32)
    for a in (X, Q):
        a.setflags(write=False)
    return X, Q


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
def test_parity(hip, mk, data, metric, storage):
    X, Q = data
    n, d, nlist = 3000, 128, 12
    rng = np.random.default_rng(12)
    h = mk(d, metric, storage=storage)
    hip.LanceDetachedAddBatch(h, X[:2500], 2500, d)
    hip.LanceDetachedDeleteBatch(h, rng.choice(2500, 100, replace=False))
    hip.LanceDetachedCreateIndex(h, nlist, 7)  # (num_sub_vectors is ignored)
    info = hip.LanceHipIvfInfo(h)
    assert info["type"] == "ivf_sq" and info["nlist"] == nlist and info["n_indexed"] == 2500
    assert info["m"] == d and info["dsub"] == 1
    hip.LanceDetachedAddBatch(h, X[2500:], 500, d)
    hip.LanceDetachedDeleteBatch(h, rng.choice(n, 60, replace=False))
    Xs = bf16_round(X) if storage == "bf16" else X
    ex = hip.LanceHipIvfExport(h)
    probing = np.bincount(sq_ref.coarse_probes(ex["centroids"], Q, metric, 6)[0].ravel(), minlength=nlist)
    assert probing.max() > 16  # some list's queries span two MFMA column groups
    for nprobe, rf, k in [(6, 2, 10), (1, 1, 5), (12, 3, 40)]:
        got = hip.LanceDetachedSearchBatch(h, Q, k, nprobes=nprobe, refine_factor=rf)
        assert_same(got, ref_search(hip, h, Xs, Q, k, nprobe, rf, metric))


# 2 ---------------------------------------------------------------------------
EDGE_SIZES = [0, 1, 64, 65, 256, 257]


@pytest.mark.parametrize("nq", [1, 17])
@pytest.mark.parametrize("d", [3, 40, 96, 200])
def test_edge_list_sizes(hip, mk, d, nq):
    rng = np.random.default_rng(100 * d + nq)
    nl = len(EDGE_SIZES)
    C = np.zeros((nl, d), np.float32)
    C[:, 0] = 10.0 * np.arange(nl)
    own = np.repeat(np.arange(nl), EDGE_SIZES)
    X = (C[own] + 0.5 * rng.standard_normal((len(own), d))).astype(np.float32)
    perm = rng.permutation(len(X))
    X, own = X[perm], own[perm]
    Q = (X[rng.choice(len(X), nq, replace=False)] + 0.3 * rng.standard_normal((nq, d))).astype(np.float32)
    h = mk(d)
    hip.LanceDetachedAddBatch(h, X, len(X), d)
    hip.LanceHipIvfSetModel(h, "ivf_sq", C, np.array([X.min(), X.max()], np.float32))
    ex = hip.LanceHipIvfExport(h)
    np.testing.assert_array_equal(ex["lists"], own)
    assert np.bincount(ex["lists"], minlength=nl).tolist() == EDGE_SIZES
    for nprobe, rf, k in [(nl, 2, 10), (2, 1, 3)]:
        got = hip.LanceDetachedSearchBatch(h, Q, k, nprobes=nprobe, refine_factor=rf)
        assert_same(got, ref_search(hip, h, X, Q, k, nprobe, rf, "l2"))


@pytest.mark.parametrize("d", [1100, 2100])  # ldc 1152, 2112
def test_wide_rows(hip, mk, d):
    # the group's query rows share LDS with the 33 KB key buffer: past d = 2040 they are the larger of the two, and
    # 40 queries on every list make three 16-query groups per block
    rng = np.random.default_rng(d)
    sizes = [70, 300]
    C = np.zeros((2, d), np.float32)
    C[1, 0] = 20.0
    own = np.repeat(np.arange(2), sizes)
    X = (C[own] + 0.5 * rng.standard_normal((len(own), d))).astype(np.float32)
    Q = (X[rng.choice(len(X), 40, replace=False)] + 0.3 * rng.standard_normal((40, d))).astype(np.float32)
    h = mk(d)
    hip.LanceDetachedAddBatch(h, X, len(X), d)
    hip.LanceHipIvfSetModel(h, "ivf_sq", C, np.array([X.min(), X.max()], np.float32))
    got = hip.LanceDetachedSearchBatch(h, Q, 10, nprobes=2, refine_factor=2)
    assert_same(got, ref_search(hip, h, X, Q, 10, 2, 2, "l2"))


def test_set_model_rejects_bad_bounds(hip, mk):
    h = mk(8)
    hip.LanceDetachedAddBatch(h, np.ones((4, 8), np.float32), 4, 8)
    C = np.ones((1, 8), np.float32)
    with pytest.raises(hip.IOException, match="bounds"):
        hip.LanceHipIvfSetModel(h, "ivf_sq", C, None)
    with pytest.raises(hip.IOException, match="bounds"):
        hip.LanceHipIvfSetModel(h, "ivf_sq", C, np.array([0.0, np.inf], np.float32))


# 3 ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_export_bounds_and_clamped_codes(hip, mk, data, metric):
    X, Q = data
    n, d, nlist = 3000, 128, 12  # nlist * 256 >= n: the sample is the table
    h = mk(d, metric)
    hip.LanceDetachedAddBatch(h, X, n, d)
    hip.LanceDetachedCreateIndex(h, nlist, 0)
    ex = hip.LanceHipIvfExport(h)
    V = sq_ref.row_values(X, metric)
    lo, hi = ex["codebook"]
    assert lo == V.min() and hi == V.max()  # (cosine: of the row-normalised values)
    np.testing.assert_array_equal(ex["codes"], sq_ref.sq_codes(X, lo, hi, metric))
    if metric != "l2":
        return
    # rows at 3x the range, indexed by compact: their codes clamp to 0 / 255
    rng = np.random.default_rng(31)
    far = (3.0 * np.where(rng.random((50, d)) < 0.5, lo, hi)).astype(np.float32)
    hip.LanceDetachedAddBatch(h, far, 50, d)
    hip.LanceDetachedCompact(h)
    ex = hip.LanceHipIvfExport(h)
    assert ex["n_indexed"] == n + 50 and (ex["lists"] >= 0).all()
    assert tuple(ex["codebook"]) == (lo, hi)
    assert set(np.unique(ex["codes"][n:]).tolist()) == {0, 255}
    Xall = np.concatenate([X, far])
    np.testing.assert_array_equal(ex["codes"], sq_ref.sq_codes(Xall, lo, hi, metric))
    Q2 = np.concatenate([Q[:8], far[:4]])
    got = hip.LanceDetachedSearchBatch(h, Q2, 10, nprobes=4, refine_factor=2)
    assert_same(got, ref_search(hip, h, Xall, Q2, 10, 4, 2, metric))


# 4 ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
def test_all_probes_against_flat_search(hip, mk, data, metric):
    X, Q = data
    n, d, nlist = 3000, 128, 12
    h = mk(d, metric)
    hip.LanceDetachedAddBatch(h, X, n, d)
    hip.LanceDetachedCreateIndex(h, nlist, 0)
    el, ed, ec = flat_knn.flat_search_batch(X, np.arange(n), np.ones(n, bool), Q, 10, metric)
    gl, _, _ = hip.LanceDetachedSearchBatch(h, Q, 10, nprobes=nlist, refine_factor=1)
    assert flat_knn.recall_at_k(gl, el, 10) >= 0.90
    got = hip.LanceDetachedSearchBatch(h, Q, 10, nprobes=nlist, refine_factor=4)
    assert_same(got, (el, ed, ec))


# 5 ---------------------------------------------------------------------------
@pytest.mark.parametrize("tie", ["label_desc", "label_asc"])
def test_ties(hip, mk, tie):
    rng = np.random.default_rng(5)
    d = 16
    same = np.tile(rng.standard_normal(d).astype(np.float32), (30, 1))
    other = (same[0] + 4.0 + rng.standard_normal((20, d))).astype(np.float32)
    X = np.concatenate([same, other])
    h = mk(d, options=[("tie", tie)])
    hip.LanceDetachedAddBatch(h, X, len(X), d)
    C = np.stack([same[0], other.mean(0)]).astype(np.float32)
    hip.LanceHipIvfSetModel(h, "ivf_sq", C, np.array([X.min(), X.max()], np.float32))
    Q = same[:2] + np.float32(0.01)
    gl, gd, gc = hip.LanceDetachedSearchBatch(h, Q, 10, nprobes=1, refine_factor=1)
    # the 10 candidates are the identical rows with the lowest labels; their final order is the handle's
    want = list(range(10)) if tie == "label_asc" else list(range(9, -1, -1))
    assert gl[0].tolist() == want and gl[1].tolist() == want and gc.tolist() == [10, 10]
    assert_same((gl, gd, gc), ref_search(hip, h, X, Q, 10, 1, 1, "l2", tie=tie))


# 6 ---------------------------------------------------------------------------
def test_predicate(hip, data):
    import pyarrow as pa

    X, Q = data
    n, d, nlist = 3000, 128, 12
    bucket = (np.arange(n) * 7 % 10).astype(np.int64)
    extras = [("bucket", pa.array(bucket, pa.int64()), None)]
    batch = hip.arrow_rows(X, extras)
    with hip.ArrowC(batch) as sch:
        h = hip.LanceCreateDetachedFromArrow("", sch.schema_ptr, "l2", "sqfilt")
    try:
        hip.LanceHipSetOption(h, "index_type", "ivf_sq")
        with hip.ArrowC(batch) as a:
            hip.LanceDetachedAddBatchArrow(h, a.schema_ptr, a.array_ptr)
        hip.LanceDetachedCreateIndex(h, nlist, 0)
        dead = np.arange(0, n, 13)
        hip.LanceDetachedDeleteBatch(h, dead)
        sel = bucket < 3
        got = hip.LanceDetachedSearchBatch(h, Q, 10, nprobes=6, refine_factor=2, predicate="bucket < 3")
        gl = got[0]
        assert sel[gl[gl >= 0]].all() and not np.isin(gl, dead).any()
        assert_same(got, ref_search(hip, h, X, Q, 10, 6, 2, "l2", selected=sel))
        before = hip.LanceHipFilterInfo(h)
        again = hip.LanceDetachedSearchBatch(h, Q, 10, nprobes=6, refine_factor=2, predicate="bucket < 3")
        after = hip.LanceHipFilterInfo(h)
        assert after["hits"] == before["hits"] + 1 and after["misses"] == before["misses"]
        for x, y in zip(got, again):
            np.testing.assert_array_equal(x, y)
    finally:
        hip.LanceFreeDetached(h)


# 7 ---------------------------------------------------------------------------
def test_index_persists_across_reopen(hip, data, tmp_path):
    X, Q = data
    d = 128
    h = hip.LanceCreateDetached(str(tmp_path), d, "l2", "t")
    hip.LanceHipSetOption(h, "index_type", "ivf_sq")
    hip.LanceDetachedAddBatch(h, X[:2000], 2000, d)
    hip.LanceDetachedCreateIndex(h, 10, 0)
    hip.LanceDetachedAddBatch(h, X[2000:2400], 400, d)
    r0 = hip.LanceDetachedSearchBatch(h, Q, 7, nprobes=3, refine_factor=2)
    i0 = hip.LanceHipIvfInfo(h)
    b0 = hip.LanceHipIvfExport(h)["codebook"].copy()
    hip.LanceFreeDetached(h)
    h2 = hip.LanceOpenDetached(str(tmp_path), "t", "l2")
    try:
        assert hip.LanceHipIvfInfo(h2) == i0 and i0["type"] == "ivf_sq"
        np.testing.assert_array_equal(hip.LanceHipIvfExport(h2)["codebook"], b0)
        r1 = hip.LanceDetachedSearchBatch(h2, Q, 7, nprobes=3, refine_factor=2)
        for x, y in zip(r0, r1):
            np.testing.assert_array_equal(x, y)
    finally:
        hip.LanceFreeDetached(h2)


# 8 ---------------------------------------------------------------------------
def test_create_hnsw_index_builds_ivf_sq(hip):
    X = hnsw_rows(256)
    h = hip.LanceCreateDetached("", 3, "l2", "hnsw")
    try:
        with pytest.raises(hip.IOException, match="create_hnsw_index failed: .*empty table"):
            hip.LanceDetachedCreateHnswIndex(h, 20, 50)
        e = hip._err()
        assert hip.lib().lance_detached_create_hnsw_index(h, 20, 50, e, hip.ERR_BUF_LEN) == -1
        assert e.value.decode().startswith("create_hnsw_index failed: ")
        hip.LanceHipSetOption(h, "index_type", "ivf_pq")  # (the option does not apply to this entry point)
        hip.LanceDetachedAddBatch(h, X, 256, 3)
        hip.LanceDetachedCreateHnswIndex(h, 20, 50)
        info = hip.LanceHipIvfInfo(h)
        assert info["type"] == "ivf_sq" and info["nlist"] == 16 and info["n_indexed"] == 256
        Q = X[[0, 17, 200]] + np.float32(0.01)
        gl, gd, gc = hip.LanceDetachedSearchBatch(h, Q, 3)
        assert gc.tolist() == [3, 3, 3] and (gl >= 0).all()
        got = hip.LanceDetachedSearchBatch(h, Q, 3, nprobes=16, refine_factor=4)
        assert_same(got, flat_knn.flat_search_batch(X, np.arange(256), np.ones(256, bool), Q, 3, "l2"))
        hip.LanceDetachedCreateHnswIndex(h, 0, 0)  # any m / ef_construction
        assert hip.LanceHipIvfInfo(h)["type"] == "ivf_sq"
    finally:
        hip.LanceFreeDetached(h)


# 9 ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["create_index", "create_hnsw_index"])
def test_two_stores_on_one_device(hip, data, entry):
    X, Q = data
    n, d = 3000, 128
    h = hip.LanceCreateDetached("", d, "l2", "t")
    try:
        hip.LanceHipSetOption(h, "devices", "0,0")
        hip.LanceHipSetOption(h, "index_type", "ivf_sq")
        for lo in range(0, n, 500):
            hip.LanceDetachedAddBatch(h, X[lo:lo + 500], 500, d)
        if entry == "create_index":
            hip.LanceDetachedCreateIndex(h, 12, 0)
        else:
            hip.LanceDetachedCreateHnswIndex(h, 20, 50)
        info = hip.LanceHipIvfInfo(h)
        assert info["type"] == "ivf_sq" and info["n_indexed"] == n
        assert info["nlist"] == (12 if entry == "create_index" else int(np.sqrt(n)))
        got = hip.LanceDetachedSearchBatch(h, Q, 10, nprobes=info["nlist"], refine_factor=4)
        assert_same(got, flat_knn.flat_search_batch(X, np.arange(n), np.ones(n, bool), Q, 10, "l2"))
    finally:
        hip.LanceFreeDetached(h)


# 10 --------------------------------------------------------------------------
def test_async_and_a_nan_query(hip, mk, data):
    import torch
    from lance_hip.sharded import AsyncPipeline

    X, Q = data
    n, d = 3000, 128
    h = mk(d)
    hip.LanceDetachedAddBatch(h, X, n, d)
    hip.LanceDetachedCreateIndex(h, 12, 0)
    sync = hip.LanceDetachedSearchBatch(h, Q, 10, nprobes=6, refine_factor=2)
    pipe = AsyncPipeline(hip.lib(), h, d, nprobes=6, refine_factor=2)
    t = pipe.submit(torch.from_numpy(np.array(Q)).cuda(), 10)
    out = tuple(x.cpu().numpy() for x in pipe.wait(t))
    for x, y in zip(sync, out):
        np.testing.assert_array_equal(x, y)
    Qn = np.array(Q)
    Qn[3, 5] = np.nan
    bad = hip.LanceDetachedSearchBatch(h, Qn, 10, nprobes=6, refine_factor=2)
    keep = np.arange(len(Q)) != 3
    for x, y in zip(sync, bad):
        np.testing.assert_array_equal(x[keep], y[keep])
