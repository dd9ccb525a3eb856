"""IVF_SQ without a GPU: properties of the numpy reference (tests/sq_ref.py) and
checks on the built sq_kernels.o (no scratch in the list scan, the MFMA operand
guard's disassembly check)."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import flat_knn
from tests import sq_ref
from tests.test_mfma_guard_cpu import _kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJS = sorted(glob.glob(os.path.join(ROOT, "duckdb-lancedb_amd", "lib", "*.o")))
LLVM = "/opt/rocm/lib/llvm/bin"


def clustered(rng, n, d, centers=48, spread=0.35):
    C = rng.standard_normal((centers, d)).astype(np.float32)
    lab = rng.integers(0, centers, n)
    return (C[lab] + spread * rng.standard_normal((n, d))).astype(np.float32)


@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
def test_reference_recall_with_every_list_probed(metric):
    rng = np.random.default_rng(1)
    n, d, nlist, nq = 3000, 128, 12, 40
    X = clustered(rng, n, d)
    Q = (X[rng.choice(n, nq, replace=False)] + 0.2 * rng.standard_normal((nq, d))).astype(np.float32)
    labels, live = np.arange(n), np.ones(n, bool)
    C = X[:nlist].copy()
    lists = rng.integers(0, nlist, n)
    V = sq_ref.row_values(X, metric)
    lo, hi = V.min(), V.max()
    el, _, _ = flat_knn.flat_search_batch(X, labels, live, Q, 10, metric)
    l1, _, c1 = sq_ref.ivf_sq_search(X, labels, live, lists, C, lo, hi, Q, 10, nlist, 1, metric)
    assert (c1 == 10).all()
    assert flat_knn.recall_at_k(l1, el, 10) >= 0.90
    l4, _, _ = sq_ref.ivf_sq_search(X, labels, live, lists, C, lo, hi, Q, 10, nlist, 4, metric)
    assert flat_knn.recall_at_k(l4, el, 10) == 1.0


def test_reference_codes_and_degenerate_bounds():
    x = np.array([[-3.0, 0.5, 1.5, 254.6, 300.0]], np.float32)
    c = sq_ref.sq_codes(x, 0.0, 255.0)  # s = 1: rint half to even, out of range clamps
    assert c.tolist() == [[0, 0, 2, 255, 255]]
    s, mid = sq_ref.sq_params(2.0, 2.0)
    assert s == 1.0 and mid == 130.0
    # a zero query: every key equals the row term (l2) / +0 (dot)
    cp = c.astype(np.int64) - 128
    rt = sq_ref.row_terms(cp, 0.0, 255.0)
    assert sq_ref.sq_keys(cp, rt, np.zeros(5, np.float32), 0.0, 255.0, "l2")[0] == rt[0]
    kd = sq_ref.sq_keys(cp, rt, np.zeros(5, np.float32), 0.0, 255.0, "dot")
    assert kd[0] == 0.0 and not np.signbit(kd[0])
    # the row term is |x~|^2 of the dequantised row x~ = mid + s c' (here exactly)
    assert rt[0] == np.float32(((c.astype(np.float64)) ** 2).sum())


needs_objs = pytest.mark.skipif(not OBJS or not os.path.exists(os.path.join(LLVM, "llvm-readelf")),
                                reason="needs the built objects (make) and the ROCm LLVM tools")


@needs_objs
def test_sq_scan_does_not_spill():
    obj = [o for o in OBJS if os.path.basename(o) == "sq_kernels.o"]
    assert obj, OBJS
    meta = _kernel_metadata(obj[0])
    scan = {k: v for k, v in meta.items() if "sq_list_scan_kernel" in k}
    assert len(scan) == 3, sorted(meta)  # l2, dot, cosine
    assert all(v[0] == 0 for v in scan.values()), scan


@needs_objs
def test_sq_kernels_pass_the_mfma_operand_check():
    obj = [o for o in OBJS if os.path.basename(o) == "sq_kernels.o"]
    assert obj, OBJS
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_mfma_war.py"), "--list", *obj],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    with_mfma = [ln for ln in r.stdout.splitlines() if "MFMAs," in ln]
    assert any(ln.startswith("sq_kernels.o") for ln in with_mfma), r.stdout[-2000:]
    assert any(ln.startswith("kernel sq_kernels.o") and "sq_list_scan_kernel" in ln for ln in r.stdout.splitlines())
