"""Pin the oracle's line-search constants against the REFERENCE's own code.

The fixtures in tests/golden/consts/ were produced by tests/golden/make_consts.py from
oracle/_ref/ref_lbfgs_<set>: the reference's sequential sources, compiled unchanged, with the
constants of one set of tests/consts_cases.py supplied through config.h's include guard. In ORC_SEQ
mode the oracle, given the same constants, must reproduce every objective call bit for bit (the
assertions of test_oracle_reproduces_reference_trace), and every fixture must differ from the
oracle's run at the default constants: one that does not pins nothing.
"""
import json
import os

import numpy as np
import pytest

import consts_cases as K
import oracle_lib as O

CONSTS_DIR = os.path.join(O.GOLDEN, "consts")


def consts_cases():
    return sorted(f[:-5] for f in os.listdir(CONSTS_DIR) if f.endswith(".json"))


def load(name):
    with open(os.path.join(CONSTS_DIR, name + ".json")) as fp:
        meta = json.load(fp)
    arr = np.load(os.path.join(CONSTS_DIR, name + ".npz"), allow_pickle=False)
    return meta, {k: arr[k] for k in arr.files}


def test_fixtures_cover_the_table():
    """every search with K1, K2 and K5 on both objectives' families, K3 and K4 where they are meant"""
    seen = {}
    for name in consts_cases():
        meta, _ = load(name)
        assert meta["consts"] == K.SETS[meta["consts_set"]], name  # the table has not moved since
        assert meta["n"] <= 1000 and meta["maxit"] <= 60
        seen.setdefault((meta["consts_set"], meta["method"]), set()).add((meta["objective"], meta["n"]))
    for ks in ("K1", "K2", "K5"):
        for ls in K.SEARCHES:
            assert len(seen[(ks, ls)]) == 2, (ks, ls)
    assert ("K3", "backtracking_wolfe") in seen
    assert {("K4", "backtracking"), ("K4", "interpolation"), ("K4", "wolfe")} <= set(seen)
    assert len(consts_cases()) >= 24


@pytest.mark.parametrize("name", consts_cases())
def test_oracle_reproduces_reference_with_constants(name):
    meta, g = load(name)
    n = meta["n"]
    assert np.all(np.isfinite(g["f_calls"]))  # the sign of a NaN is the processor's choice
    x0 = O.x0_uniform(n, meta["seed"], meta["lo"], meta["hi"])
    args = (meta["objective"], x0, meta["method"], meta["m"], meta["maxit"], meta["tol"])
    r = O.lbfgs(*args, mode=O.SEQ, consts=meta["consts"], log_calls=True)
    # every f() value, in call order
    ref_f = g["f_calls"]
    assert len(r["flog"]) == len(ref_f)
    assert np.array_equal(r["flog"].view(np.uint64), ref_f.view(np.uint64))
    # every grad() argument (checksums) and |grad| (bits)
    ref_gc, ref_gn = g["grad_c"], g["grad_norm"]
    assert r["glog"].shape[0] == ref_gc.shape[0]
    assert np.array_equal(r["glog"][:, 0:2], ref_gc)
    assert np.array_equal(r["glog"][:, 2], ref_gn.view(np.uint64))
    # returned x
    assert O.checksum(r["x"]) == tuple(int(v) for v in g["ret_c"])
    assert np.array_equal(r["x"].view(np.uint64), g["ret_x"].view(np.uint64))
    # messages (the reference's non-verbose stdout)
    assert r["messages"] == meta["stdout"]
    # the constants bite: the default constants give another sequence of f-calls
    d = O.lbfgs(*args, mode=O.SEQ, log_calls=True)
    assert not (len(d["flog"]) == len(ref_f) and np.array_equal(d["flog"].view(np.uint64), ref_f.view(np.uint64)))
