"""Histories of 17 to 64 pairs on the single-problem paths.

lbfgs_ctx_create accepts m up to 64 (MMAX). The cooperative one-launch iteration and the persistent
two-loop stop at 16 pairs (LBK_SMALL_HMAX), so a small-n solve with m > 16 starts on the cooperative
iteration, with the next one queued ahead, and in mid-solve, at the first iteration that has 17 pairs,
moves to the launch sequence (twoloop_passes); its device-resident line searches stay cooperative. This
file runs that hand-over and everything behind it that is sized by m: the result slots up to
SLOT_MISC(64), the pool of 65 pairs and its rotation, the carried s.g of the commit before the crossing,
the queued launch that must not be made at 17 pairs, the knobs that change where a stage 2 runs, the
paths that never go cooperative (unfused, host callbacks, the CUDA path's loop), larger n and sharded
ranks. Bits are compared throughout, with the canonical-order oracle or with the default run.

The inputs are tests/hist_cases.py's SINGLE_LONG and SINGLE_LONG_LARGE; what the tests rely on (the
ring fills and rotates, searches go past their first trial at more than 16 pairs) is asserted on the
oracle alone in tests/test_history_inputs.py.
"""
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-lbfgs_amd"))
import lbfgs_amd as L  # noqa: E402
import oracle_lib as O  # noqa: E402
import hist_cases as HC  # noqa: E402
from test_gpu_knobs import KNOBS, VARIANTS  # noqa: E402

pytestmark = pytest.mark.gpu

HMAX = 16  # LBK_SMALL_HMAX: the cooperative iteration's and the persistent two-loop's limit


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    """every run starts from the default path: the knobs are read at creation and per solve"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_as_oracle(r, o, what):
    assert r["status"] == o["status"] and r["iterations"] == o["iters"], (what, r["status"], r["iterations"])
    for key in ("f", "gnorm", "alpha"):
        assert HC.same_bits(r["tr_" + key], o[key]), (what, key)
    assert np.array_equal(r["tr_c1"], o["c1"]) and np.array_equal(r["tr_c2"], o["c2"]), what
    assert HC.same_bits(r["x"], o["x"]), what
    assert r["messages"] == o["messages"], what


def same_runs(a, b, what):
    """test_gpu_knobs.py's comparison of a variant with the default run"""
    assert np.all(np.isfinite(b["tr_f"])) and np.all(np.isfinite(b["tr_gnorm"])), what
    for key in ("tr_f", "tr_gnorm", "x"):
        assert np.array_equal(bits(a[key]), bits(b[key])), (what, key)
    ta, tb = a["tr_alpha"], b["tr_alpha"]
    assert np.array_equal(np.isnan(ta), np.isnan(tb)) and np.array_equal(ta[~np.isnan(ta)], tb[~np.isnan(tb)]), what
    assert np.array_equal(a["tr_c1"], b["tr_c1"]) and np.array_equal(a["tr_c2"], b["tr_c2"]), what
    assert a["messages"] == b["messages"] and a["status"] == b["status"] and a["iterations"] == b["iterations"], what


def solve(case, **kw):
    n, m, ls, it = case
    with L.Context(n, m) as c:
        return c.minimize("rosenbrock", HC.long_x0(n), ls, it, tolerance=HC.LONG_TOL, trace=True, **kw)


_default = {}


def default_run(case):
    """the default path's traced run of a case, computed once (under no_knobs) and left unchanged"""
    if case not in _default:
        _default[case] = solve(case)
    return _default[case]


# ---- a. parity with the oracle; f. larger n ----
@pytest.mark.parametrize("case", HC.SINGLE_LONG + HC.SINGLE_LONG_LARGE, ids=HC.long_id)
def test_long_history_parity(case):
    n, m, ls, it = case
    r = default_run(case)
    same_as_oracle(r, HC.long_oracle(case), case)
    assert r["h_max"] == m and r["h_min"] == 0, (case, r["h_min"], r["h_max"])


# ---- b. the crossing from the cooperative iteration to the launch sequence; c. device searches ----
_stepped = {}


def stepped(case):
    """The case through the stepping API with profiling on. Calls of one iteration cannot queue the next
    one (nothing is queued past the last step of a call), so the calls take two iterations wherever both
    are on the same side of the crossing: two while the last iteration seen had at most 14 pairs (the
    next two have at most 16), one until an iteration has had 17, two from then on. No call straddles the
    crossing, whatever updates are skipped. One record per call, read after it."""
    if case in _stepped:
        return _stepped[case]
    n, m, ls, it = case
    rec = []
    with L.Context(n, m) as c:
        c.prof_reset()
        c.prof_enable(True)
        c.init("rosenbrock", HC.long_x0(n), ls, tolerance=HC.LONG_TOL)
        done, h_top = 0, -1
        while done < it:
            steps = 1 if done == 0 or HMAX - 2 < h_top <= HMAX else min(2, it - done)
            r = c.step(steps)
            assert r["status"] == "running" and r["iterations"] == done + steps, (case, r)
            done, h_top = r["iterations"], r["h_max"]
            rec.append(dict(k=done, h_min=r["h_min"], h_max=r["h_max"], spec=c.spec_stats(), search=c.search_stats(),
                            small=c.prof_get("small_iter")["launches"], axpy=c.prof_get("axpy_dot")["launches"]))
        c.prof_enable(False)
        out = dict(rec=rec, x=c.get_x(), f=r["f"], gnorm=r["gnorm"], coop=c.coop_info())
    _stepped[case] = out
    return out


def crossing(rec):
    """index of the first call whose iterations have 17 pairs or more"""
    j = next(i for i, q in enumerate(rec) if q["h_min"] > HMAX)
    assert j > 0 and rec[j - 1]["h_max"] == HMAX and rec[j]["h_min"] == HMAX + 1, (rec[j - 1], rec[j])
    return j


CROSSING = [c for c in HC.SINGLE_LONG if c[0] in (513, 1537) and c[1] in (17, 64)]


@pytest.mark.parametrize("case", CROSSING, ids=HC.long_id)
def test_crossing_to_the_launch_sequence(case):
    n, m, ls, it = case
    s = stepped(case)
    rec, j = s["rec"], crossing(s["rec"])
    nseg = O.geometry(n)[1]
    assert s["coop"]["coop_max"] >= nseg, s["coop"]
    print(f"{HC.long_id(case)}: first iteration with 17 pairs k = {rec[j - 1]['k']}; before it small_iter "
          f"{rec[j - 1]['small']}, axpy_dot {rec[j - 1]['axpy']}, adopted/dropped {rec[j - 1]['spec']}, searches "
          f"{rec[j - 1]['search']}; at the end small_iter {rec[-1]['small']}, axpy_dot {rec[-1]['axpy']}, "
          f"adopted/dropped {rec[-1]['spec']}, searches {rec[-1]['search']}")
    # 1 <= h <= 16: every call launches the cooperative iteration, and queued launches were taken
    for a, b in zip(rec[:j], rec[1:j]):
        assert b["h_min"] >= 1 and b["small"] > a["small"], (a, b)
    assert rec[j - 1]["spec"][0] > 0, rec[j - 1]
    # h >= 17: no cooperative iteration, nothing queued, taken or dropped; the launch sequence's passes
    for a, b in zip(rec[j - 1:], rec[j:]):
        assert b["small"] == rec[j - 1]["small"] and sum(b["spec"]) == sum(rec[j - 1]["spec"]), (a, b)
        assert b["axpy"] > a["axpy"], (a, b)
    assert rec[-1]["h_max"] == m
    # stepping and profiling change no bit
    one = default_run(case)
    assert HC.same_bits(s["x"], one["x"]) and HC.same_bits([s["f"], s["gnorm"]], [one["f"], one["gnorm"]]), case
    with L.Context(n, m) as c:
        c.prof_enable(True)
        prof = c.minimize("rosenbrock", HC.long_x0(n), ls, it, tolerance=HC.LONG_TOL, trace=True)
        c.prof_enable(False)
    same_runs(one, prof, case)


def searches_past_16(case):
    """device line-search launches of the iterations with 17 pairs or more"""
    rec = stepped(case)["rec"]
    j = crossing(rec)
    return rec[-1]["search"][0] - rec[j - 1]["search"][0]


def test_device_search_beyond_16_pairs():
    """A launch-sequence two-loop followed by a cooperative search and commit: the cases of
    hist_cases.LONG_DEVICE_SEARCH, and only they, continue a line search on the device while more than
    16 pairs are stored; every line search has one."""
    got = {case: searches_past_16(case) for case in HC.SINGLE_LONG}
    for case in HC.SINGLE_LONG:
        print(f"{HC.long_id(case)}: {got[case]} device searches at 17 pairs or more")
    assert {case for case, k in got.items() if k > 0} == set(HC.LONG_DEVICE_SEARCH)
    assert {c[2] for c in HC.LONG_DEVICE_SEARCH} == set(HC.SEARCHES)
    for case in HC.LONG_DEVICE_SEARCH:  # the stepped run is the oracle's
        s, o = stepped(case), HC.long_oracle(case)
        assert HC.same_bits(s["x"], o["x"]) and HC.same_bits([s["f"], s["gnorm"]], [o["f"][-1], o["gnorm"][-1]]), case


# ---- d. knobs ----
KNOB_CASES = [(513, 64, "wolfe", 80), (1537, 17, "backtracking", 30), (1537, 64, "interpolation", 80),
              (100_003, 64, "backtracking_wolfe", 80)]
LONG_VARIANTS = {k: VARIANTS[k] for k in (
    "coop0", "spec0", "devsearch0", "devsearch0_spec0", "batch0", "coop0_spec0_batch0", "ticket0", "ticket1", "defer0",
    "defer_all", "direct0", "persist2", "persist2_coop0_nt1", "search_timeout0")}
# the reduce-kernel stage 2 at a few segments
LONG_VARIANTS["coop0_ticket0_defer0"] = {"LBFGS_COOP": "0", "LBFGS_TICKET": "0", "LBFGS_DEFER": "0"}


@pytest.mark.parametrize("variant", sorted(LONG_VARIANTS))
@pytest.mark.parametrize("case", KNOB_CASES, ids=HC.long_id)
def test_long_history_knob_bit_identical(monkeypatch, case, variant):
    assert case in HC.SINGLE_LONG + HC.SINGLE_LONG_LARGE
    a = default_run(case)
    for k, v in LONG_VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    same_runs(a, solve(case), (case, variant))


# ---- e. paths that never go cooperative: n = 513, m = 64, 80 iterations ----
@pytest.mark.parametrize("ls", HC.SEARCHES)
def test_long_history_unfused(ls):
    case = (513, 64, ls, 80)
    same_runs(default_run(case), solve(case, unfused=True), case)


@pytest.mark.parametrize("reference_calls", [False, True], ids=["one_call_per_point", "reference_calls"])
@pytest.mark.parametrize("ls", ["backtracking", "wolfe"])
def test_long_history_host_callbacks(ls, reference_calls):
    case = (513, 64, ls, 80)
    cb = HC.Callables("rosenbrock")
    with L.Context(513, 64) as c:
        r = c.minimize("host", HC.long_x0(513), ls, 80, tolerance=HC.LONG_TOL, trace=True, f=cb.f, grad=cb.grad,
                       reference_calls=reference_calls)
    same_runs(default_run(case), r, case)
    assert r["h_max"] == 64


@pytest.mark.parametrize("cuda", [1, 2], ids=["cuda_compat", "cuda_variant"])
@pytest.mark.parametrize("ls", HC.SEARCHES)
def test_long_history_cuda_path(ls, cuda):
    """cu_alpha[MMAX] / cu_rho[MMAX] and the ring slot k % m, which wraps at k = 64"""
    n, m, it = 513, 64, 80
    x0 = HC.long_x0(n)
    o = HC.long_cuda_oracle(ls, cuda)
    with L.Context(n, m) as c:
        r = c.minimize("rosenbrock", x0, ls, it, tolerance=HC.LONG_TOL, trace=True, cuda_compat=True,
                       cuda_variant=cuda == 2, consts=L.constants("cuda"))
    assert r["status"] == o["status"] and r["iterations"] == o["iters"]
    for key in ("f", "gnorm", "alpha"):
        assert np.array_equal(bits(r["tr_" + key]), bits(o[key])), key
    assert np.array_equal(r["tr_c1"], o["c1"]) and np.array_equal(r["tr_c2"], o["c2"])
    assert np.array_equal(bits(r["x"]), bits(o["x"]))
    assert r["messages"] == o["messages"]


# ---- g. sharded ranks: 2 m exchanges per iteration ----
@pytest.mark.parametrize("world", [2, 8])
def test_long_history_sharded_emulated(world):
    """test_gpu_parity.py's test_sharded_emulated_bit_exact at m = 24, 30 iterations"""
    n, m, ls, it = 4_000_003, 24, "wolfe", 30
    x0 = HC.long_x0(n)
    ref = default_run((n, m, ls, it))
    assert ref["h_max"] == m
    grp = L.HostGroup(world)
    ctxs = [L.Context(n, m, rank=r, group=grp) for r in range(world)]
    out, err = [None] * world, [None] * world

    def run(r):
        try:
            out[r] = ctxs[r].minimize("rosenbrock", x0, ls, it, tolerance=HC.LONG_TOL, trace=True)
        except Exception as e:  # pragma: no cover
            err[r] = e

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    assert not any(err), err
    x = np.zeros(n)
    for r in range(world):
        o = out[r]
        for key in ["tr_f", "tr_gnorm", "tr_alpha"]:
            assert np.array_equal(bits(o[key]), bits(ref[key])), (r, key)
        assert np.array_equal(o["tr_c1"], ref["tr_c1"]) and np.array_equal(o["tr_c2"], ref["tr_c2"])
        lo, nl = ctxs[r].elem_lo, ctxs[r].n_loc
        x[lo:lo + nl] = o["x"][lo:lo + nl]
    assert np.array_equal(bits(x), bits(ref["x"]))
    for c in ctxs:
        c.close()
    grp.close()


# ---- h. limits ----
def test_history_length_limits():
    with pytest.raises(L.LbfgsError, match=r"\(-1\)"):
        L.Context(100, 65)
    x0 = HC.long_x0(100)
    with L.Context(100, 64) as c:
        r = c.minimize("rosenbrock", x0, "backtracking", 3, tolerance=HC.LONG_TOL, trace=True)
    same_as_oracle(r, O.lbfgs("rosenbrock", x0, "backtracking", 64, 3, HC.LONG_TOL, mode=O.CANON), "m = 64")
    assert r["iterations"] == 3
