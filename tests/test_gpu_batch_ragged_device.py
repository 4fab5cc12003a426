"""Ragged batches with x0, x, A and b in device memory (lbfgs_batch_minimize_device and
lbfgs_batch_set_dense_quadratics_device on a batch made by lbfgs_batch_create_ragged) and their torch
front end, on the GPU. Everything compares bits. The cases themselves are in
tests/batch_ragged_dev_cases.py:

1. the stencil objectives on padded rows (B, n_max + 3) at storage offset 1 and on packed 1-D tensors,
   apart and in place: NaN around the inputs, a sentinel around the outputs, against the oracle and
   Batch.minimize of the same object;
2. dense quadratics by reference: (B, W, W) at batch stride W * W + 5 and packed A, padded and packed b
   in every mix, the tensors overwritten in place between solves;
3. two workgroups for seven problems, in place;
4. the refusals, each a status or an exception with nothing launched.

Why a process of its own: a torch wheel brings its own copy of the HIP runtime, and sharing device
memory between torch and the library needs both on ONE runtime (see test_gpu_batch_device.py). The
cases run once, together, in a child pytest that imports torch first; every test below reports one
function of that run.
"""
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "batch_ragged_dev_cases.py")

# test function of the child run -> its number of cases
FUNCTIONS = {
    "test_padded_rows_and_packed": 12,
    "test_dense_by_reference": 4,
    "test_two_workgroups_for_seven_problems_in_place": 1,
    "test_refusals": 1,
}


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    xml = tmp_path_factory.mktemp("batchragdev") / "cases.xml"
    p = subprocess.run([sys.executable, "-m", "pytest", CASES, "-q", "-p", "no:cacheprovider", f"--junitxml={xml}"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
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
