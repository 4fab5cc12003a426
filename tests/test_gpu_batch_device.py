"""The batched solver with x0, x, A and b in device memory (lbfgs_batch_minimize_device,
lbfgs_batch_set_dense_quadratics_device) and its torch front end (Batch.minimize_device,
Batch.set_dense_quadratics_device), on the GPU. Everything compares bits. The cases themselves are
in tests/batchdev_gpu_cases.py:

1. the stencil objectives with x0 and x as rows of a caller's buffer: contiguous, padded at storage
   offset 1, a broadcast x0, and the result over x0, against the oracle and Batch.minimize;
2. dense quadratics by reference: padded rows, padded matrices, a shared matrix through expand and
   through a 2-D tensor, a shared b, against the oracle and set_dense_quadratics + minimize;
3. by reference: the tensors overwritten in place between solves, the setters alternating, a stencil
   solve in between;
4. launch shapes (two workgroups for seven problems, also in place) and tensors from a side stream;
5. the refusals, each a status or an exception with nothing launched.

Why a process of its own: a torch wheel brings its own copy of the HIP runtime, and sharing device
memory between torch and the library needs both on ONE runtime (see test_gpu_device_objective.py).
These cases run once, together, in a child pytest that imports torch first; every test below
reports one function of that run.
"""
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "batchdev_gpu_cases.py")

# test function of the child run -> its number of cases
FUNCTIONS = {
    "test_stencil_rows": 12,
    "test_dense_rows": 12,
    "test_by_reference": 1,
    "test_launch_shape_does_not_matter": 2,
    "test_tensors_from_a_side_stream": 1,
    "test_refusals": 1,
}


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    xml = tmp_path_factory.mktemp("batchdev") / "cases.xml"
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
