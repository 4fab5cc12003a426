"""The row reducer (lbfgs_reduce_rows, lbfgs_amd.reduce_rows) on the GPU: the canonical fixed-order sum
of every row of a table in one launch, for batch callbacks. Everything compares bits. The cases
themselves are in tests/reduce_rows_gpu_cases.py:

1. against the oracle's canonical dot and the single-vector reducer, over sizes around every boundary
   of the order and layouts that make rows 16-byte aligned, 8-byte aligned, or alternate;
2. the inputs can tell the canonical order from the left-to-right one (on the CPU);
3. a mask: inactive rows are neither read nor written;
4. signed zeros;
5. stream order with no synchronisation, on a side stream and on the null stream;
6. 5000 rows;
7. end to end: a batch callback with one reduce_rows per round against the single path;
8. refusals through Python.

They run once, together, in a child pytest that imports torch first (tests/test_gpu_device_objective.py
says why); every test below reports one function of that run.
"""
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "reduce_rows_gpu_cases.py")

# test function of the child run -> its number of cases
FUNCTIONS = {
    "test_reduce_rows_vs_oracle_and_reducer": 15,
    "test_orders_differ": 1,
    "test_mask": 3,
    "test_signed_zeros": 5,
    "test_stream_order": 2,
    "test_many_rows": 1,
    "test_batch_callback_with_reduce_rows_vs_single": 4,
    "test_refusals": 1,
}


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    xml = tmp_path_factory.mktemp("reduce_rows") / "cases.xml"
    p = subprocess.run([sys.executable, "-m", "pytest", CASES, "-q", "-p", "no:cacheprovider", f"--junitxml={xml}"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    tail = p.stdout[-3000:] + p.stderr[-2000:]
    results = {}
    if os.path.exists(xml):
        for case in ET.parse(xml).getroot().iter("testcase"):
            bad = [e for e in case if e.tag in ("failure", "error", "skipped")]
            results[case.get("name")] = None if not bad else f"{bad[0].tag}: {(bad[0].text or bad[0].get('message'))}"
    return dict(rc=p.returncode, tail=tail, results=results)


@pytest.mark.parametrize("name", sorted(FUNCTIONS))
def test_cases(child, name):
    cases = {k: v for k, v in child["results"].items() if k.split("[")[0] == name}
    assert len(cases) == FUNCTIONS[name], (sorted(cases), child["rc"], child["tail"])
    bad = {k: v for k, v in cases.items() if v is not None}
    assert not bad, "\n\n".join(f"{k}\n{v[-3000:]}" for k, v in bad.items())
