"""CPU checks of the predicate program (``csrc/filter_program.h``: the flat
postfix form of a Lance-SQL predicate and the per-row interpreter the device
evaluator runs) through ``lance_hip_predicate_mask_program`` — no device.

A predicate that compiles must give, byte for byte, the mask of the vectorised
host evaluator (``lance_hip_predicate_mask``) and of ``oracle/predicate.py``; one
that does not compile must be one the program may refuse (strings, a type
pairing the evaluator rejects).  Table and generator shapes follow
``tests/test_predicate_cpu.py`` with int64 values near +-2^62 (exact compares
past 2^53), NaN / +-inf floats and an all-NULL column added."""
import ctypes
import math

import numpy as np
import pyarrow as pa
import pytest

import lance_hip
from oracle import predicate as P

BIG = 1 << 62
NOT_DEV = "predicate: not device-evaluable"


def _table(rng, n):
    def nulls(vals, p=0.15):
        return [None if rng.random() < p else v for v in vals]

    words = ["en", "fr", "es", "it's", "", "de", "EN", "zz"]
    specials = [math.nan, math.inf, -math.inf]
    f64 = rng.normal(0, 10, n).tolist()
    for i in range(n):
        if rng.random() < 0.12:
            f64[i] = specials[int(rng.integers(0, 3))]
    cols = {
        "i32": nulls(rng.integers(-50, 50, n).tolist()),
        "i64": nulls((rng.integers(-3, 3, n) * 10**12).tolist()),
        "big": nulls([int(s) * BIG + int(o) for s, o in zip(rng.choice([-1, 1], n), rng.integers(-2, 3, n))]),
        "f32": nulls([float(np.float32(x)) for x in rng.normal(0, 10, n)]),
        "f64": nulls(f64),
        "flag": nulls(rng.random(n).astype(bool).tolist()),
        "nul": [None] * n,
        "lang": nulls([words[i] for i in rng.integers(0, len(words), n)]),
    }
    types = {"i32": pa.int32(), "i64": pa.int64(), "big": pa.int64(), "f32": pa.float32(), "f64": pa.float64(),
             "flag": pa.bool_(), "nul": pa.int32(), "lang": pa.string()}
    return cols, types


NUMERIC = ["i32", "i64", "big", "f32", "f64", "nul", "label"]
COLUMNS = NUMERIC + ["flag", "lang"]


def _lit(rng, col):
    if col in ("i32", "label", "nul"):
        return str(int(rng.integers(-60, 60)))
    if col == "i64":
        return str(int(rng.integers(-3, 3)) * 10**12)
    if col == "big":
        if rng.random() < 0.25:  # a float literal: the column compares as (double)
            return repr(float(int(rng.choice([-1, 1])) * BIG))
        return str(int(rng.choice([-1, 1])) * BIG + int(rng.integers(-2, 3)))
    if col in ("f32", "f64"):
        if rng.random() < 0.2:  # an integer literal against a float column
            return str(int(rng.integers(-20, 20)))
        return repr(round(float(rng.normal(0, 10)), 3))
    if col == "flag":
        return "true" if rng.random() < 0.5 else "false"
    w = ["en", "fr", "es", "it''s", "", "de", "EN", "zz", "e"][int(rng.integers(0, 9))]
    return f"'{w}'"


def _atom(rng):
    col = COLUMNS[int(rng.integers(0, len(COLUMNS)))]
    r = rng.random()
    if r < 0.45:
        op = ["=", "!=", "<", "<=", ">", ">="][int(rng.integers(0, 6))]
        if col == "flag":
            op = ["=", "!="][int(rng.integers(0, 2))]
        a, b = col, _lit(rng, col)
        return f"{b} {op} {a}" if rng.random() < 0.2 else f"{a} {op} {b}"
    if r < 0.55 and col in NUMERIC:  # column against column
        other = NUMERIC[int(rng.integers(0, len(NUMERIC)))]
        op = ["=", "!=", "<", "<=", ">", ">="][int(rng.integers(0, 6))]
        return f"{col} {op} {other}"
    if r < 0.68:
        return f"{col} IS {'NOT ' if rng.random() < 0.5 else ''}NULL"
    if r < 0.86:
        vals = [_lit(rng, col) for _ in range(int(rng.integers(1, 4)))]
        if rng.random() < 0.2:
            vals.append("NULL")
        return f"{col} {'NOT ' if rng.random() < 0.3 else ''}IN ({', '.join(vals)})"
    if col == "flag":
        return "flag"
    lo, hi = _lit(rng, col), _lit(rng, col)
    return f"{col} {'NOT ' if rng.random() < 0.2 else ''}BETWEEN {lo} AND {hi}"


def _pred(rng, depth=0):
    r = rng.random()
    if depth >= 2 or r < 0.4:
        return _atom(rng)
    if r < 0.55:
        return f"NOT ({_pred(rng, depth + 1)})"
    if r < 0.62:
        return f"({_pred(rng, depth + 1)}) IS {'NOT ' if rng.random() < 0.5 else ''}NULL"
    if r < 0.8:
        return f"{_pred(rng, depth + 1)} AND {_pred(rng, depth + 1)}"
    return f"({_pred(rng, depth + 1)}) OR ({_pred(rng, depth + 1)})"


def _program(batch, labels, live, pred):
    """The program's mask, or None when the predicate is not device-evaluable."""
    try:
        return lance_hip.LanceHipPredicateMaskProgram(batch, labels, live, pred)
    except lance_hip.IOException as e:
        assert str(e).startswith("Lance predicate: " + NOT_DEV), (pred, str(e))
        return None


class _Case:
    def __init__(self, seed, n):
        rng = np.random.default_rng(seed)
        self.cols, types = _table(rng, n)
        X = rng.standard_normal((n, 4)).astype(np.float32)
        self.batch = lance_hip.arrow_rows(X, [(k, self.cols[k], types[k]) for k in self.cols])
        self.labels = np.arange(n, dtype=np.int64) * 2 + 3
        self.live = (rng.random(n) > 0.1).astype(np.uint8)


@pytest.fixture(scope="module")
def cases():
    return [_Case(11, 600), _Case(12, 357)]


def test_random_predicates_program_matches_host_evaluator_and_oracle(cases):
    rng = np.random.default_rng(2024)
    preds = [_pred(rng) for _ in range(400)]
    routed = 0
    for pred in preds:
        took = set()
        for c in cases:
            got = _program(c.batch, c.labels, c.live, pred)
            took.add(got is not None)
            if got is None:
                # only what the program may refuse: strings (this generator makes no other refusal)
                assert "lang" in pred or "'" in pred, pred
                continue
            host = lance_hip.LanceHipPredicateMask(c.batch, c.labels, c.live, pred)
            assert got.tobytes() == host.tobytes(), pred
            assert got.tolist() == P.mask(pred, c.cols, c.labels, c.live), pred
        assert len(took) == 1, pred  # the route depends on the predicate and the schema, not on the rows
        routed += took.pop()
    # a condition of the test's worth, not a measurement: most predicates must take the program route
    assert routed >= len(preds) // 2, routed


FIXED = [f"{col} {op} {lit}" for col, lit in [("i32", "7"), ("i32", "7.5"), ("f64", "3"), ("f64", "-1.25"),
                                               ("big", str(BIG + 1)), ("big", repr(float(BIG)))]
         for op in ["=", "!=", "<>", "<", "<=", ">", ">=", "=="]]
FIXED += [f"flag {op} {lit}" for op in ["=", "!="] for lit in ["true", "FALSE"]]
FIXED += [
    "7 < i32", "-3.5 >= f64", f"{-BIG} = big", "true = flag",
    "NOT (i32 IS NULL)", "NOT (NOT (f64 IS NOT NULL))", "nul IS NULL", "nul IS NOT NULL", "nul = 1", "nul IN (1, 2)",
    "i32 NOT IN (1, NULL)", "i32 IN (1, NULL)", "i32 IN (NULL)", "f64 IN (1, 2.5, NULL)", "i32 IN (1, 2.5, -7)",
    "flag IN (true)", "flag NOT IN (false, NULL)", "i32 IN (f64, 3, label)", "3 IN (i32, 4)",
    "(i32 < 1) IS NULL", "(i32 < 1) IS NOT NULL", "(i32 < 1 OR nul = 2) IS NULL", "(NULL = 1) IS NULL",
    "i32 BETWEEN -10 AND 10", "i32 NOT BETWEEN -10 AND 10", "f64 BETWEEN -1.5 AND 20", "label BETWEEN 100 AND 163",
    "f64 NOT BETWEEN 0 AND 1e300", "big BETWEEN -1 AND 4611686018427387904",
    "label >= 131", "label < 67 OR label > 1100", "label = 5", "label != 5", "label IN (3, 5, 7, 1201)",
    "I32 < 9", "i32 < f64", "big = big", "i64 >= i32", "f32 != f64", "flag = flag", "label > i32",
    "f64 > 1e308", "f64 >= f64", "f64 = f64", "f64 < -1e308",
    "flag", "NOT flag", "flag AND i32 > 0", "true", "false", "NULL", "NOT NULL", "1 = 1", "1 < 2.5", "NULL = 1",
    "true = true", "NULL IS NULL", "3 IS NOT NULL",
    "i32 > 0 AND (f64 < 0 OR flag) AND NOT (big < 0) AND label < 1000 OR nul IS NULL AND i64 = 0",
]


@pytest.mark.parametrize("pred", FIXED)
def test_fixed_predicates_take_the_program_route(cases, pred):
    for c in cases:
        got = lance_hip.LanceHipPredicateMaskProgram(c.batch, c.labels, c.live, pred)
        assert got.tobytes() == lance_hip.LanceHipPredicateMask(c.batch, c.labels, c.live, pred).tobytes()
        # (unquoted identifiers fold to the column's case; the oracle takes the exact name)
        assert got.tolist() == P.mask(pred.replace("I32", "i32"), c.cols, c.labels, c.live)


def test_exact_int64_compares_past_2_53(cases):
    # +-2^62 + {-2..2} are five distinct integers with one double: an exact compare tells them apart,
    # a float literal compares (double)i and does not
    c = cases[0]
    big = np.array([v if v is not None else 0 for v in c.cols["big"]], dtype=object)
    ok = np.array([v is not None for v in c.cols["big"]]) & c.live.astype(bool)
    exact = lance_hip.LanceHipPredicateMaskProgram(c.batch, c.labels, c.live, f"big = {BIG + 1}")
    assert exact.tolist() == [bool(o and v == BIG + 1) for v, o in zip(big, ok)]
    assert 0 < exact.sum() < (ok & (big > 0)).sum()
    as_double = lance_hip.LanceHipPredicateMaskProgram(c.batch, c.labels, c.live, f"big = {float(BIG)!r}")
    assert as_double.tolist() == [bool(o and v > 0) for v, o in zip(big, ok)]


def test_long_in_list_works_by_either_route(cases):
    c = cases[0]
    want = [int(x) for x in c.labels[::3]] + list(range(100000, 100000 + 800))
    pred = "label IN (" + ", ".join(map(str, want)) + ")"
    exp = [bool(l) and int(lab) in set(want) for lab, l in zip(c.labels, c.live)]
    assert lance_hip.LanceHipPredicateMask(c.batch, c.labels, c.live, pred).tolist() == exp
    got = _program(c.batch, c.labels, c.live, pred)
    assert got is not None and got.tolist() == exp
    # past the literal limit the program refuses and the host evaluator serves it
    huge = "label IN (" + ", ".join(map(str, range(5000))) + ")"
    assert _program(c.batch, c.labels, c.live, huge) is None
    assert lance_hip.LanceHipPredicateMask(c.batch, c.labels, c.live, huge).tolist() == \
        [bool(l) and int(lab) < 5000 for lab, l in zip(c.labels, c.live)]


@pytest.mark.parametrize("pred", ["lang = 'en'", "lang IS NULL", "i32 = 'a'", "i32 < 3 AND lang != 'fr'",
                                  "lang IN ('en', 'fr')", "'a' = 'a'", "flag = 1", "i32 = true", "flag < i32",
                                  "i32", "3", "(i32 < 3) = true", "i32 IN (1, 'x')"])
def test_refused_predicates_keep_the_host_evaluators_answer(cases, pred):
    c = cases[0]
    with pytest.raises(lance_hip.IOException, match="^Lance predicate: " + NOT_DEV):
        lance_hip.LanceHipPredicateMaskProgram(c.batch, c.labels, c.live, pred)
    try:  # whatever the host evaluator says (a mask or its error) is what a search would get
        host = lance_hip.LanceHipPredicateMask(c.batch, c.labels, c.live, pred)
    except lance_hip.IOException as e:
        assert NOT_DEV not in str(e)
    else:
        assert host.tolist() == P.mask(pred, c.cols, c.labels, c.live)


@pytest.mark.parametrize("bad", ["nosuchcol = 1", "i32 = ", "lang = 'x", "(i32 = 1", "i32 === 1", "i32 < 1 AND nosuch IS NULL"])
def test_syntax_errors_and_unknown_columns_are_reported_as_by_the_host_evaluator(cases, bad):
    c = cases[1]
    msgs = []
    for fn in (lance_hip.LanceHipPredicateMask, lance_hip.LanceHipPredicateMaskProgram):
        with pytest.raises(lance_hip.IOException) as ei:
            fn(c.batch, c.labels, c.live, bad)
        msgs.append(str(ei.value))
    assert msgs[0] == msgs[1]
    assert NOT_DEV not in msgs[1]


def _null_call(name, *args):
    L = lance_hip.lib()
    e = ctypes.create_string_buffer(2048)
    r = getattr(L, name)(None, *args, e, 2048)
    return r, e.value.decode()


def test_null_handle_conventions_of_the_filter_symbols():
    q = np.zeros(3, np.float32)
    lab = np.zeros(4, np.int64)
    dist = np.zeros(4, np.float32)
    cnt = np.zeros(1, np.int32)
    m = np.zeros(4, np.uint8)
    assert _null_call("lance_hip_filter_prepare", b"label < 3") == (-1, "null handle")
    assert _null_call("lance_hip_filter_mask", b"label < 3", m.ctypes.data, 4) == (-1, "null handle")
    assert _null_call("lance_hip_search_batch_device_filtered", q.ctypes.data, 1, 3, 4, 20, 1, b"label < 3",
                      lab.ctypes.data, dist.ctypes.data, cnt.ctypes.data) == (-1, "null handle")
    assert _null_call("lance_hip_search_batch_device_filtered", q.ctypes.data, 1, 3, 4, 20, 1, None,
                      lab.ctypes.data, dist.ctypes.data, cnt.ctypes.data) == (-1, "null handle")
    out = np.zeros(7, np.int64)
    L = lance_hip.lib()
    assert L.lance_hip_filter_info(None, out.ctypes.data, 7) == -1
    with pytest.raises(lance_hip.IOException, match="^Lance filter_prepare: null handle"):
        lance_hip.LanceHipFilterPrepare(None, "label < 3")
    with pytest.raises(lance_hip.IOException, match="^Lance filter_mask: null handle"):
        lance_hip.LanceHipFilterMask(None, "label < 3")
    with pytest.raises(lance_hip.IOException, match="^Lance filter_info"):
        lance_hip.LanceHipFilterInfo(None)
    e = ctypes.create_string_buffer(2048)
    assert L.lance_hip_predicate_mask_program(None, None, None, None, b"true", None, e, 2048) == -1
    assert e.value == b"predicate failed: null argument"
