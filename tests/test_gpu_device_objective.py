"""Device-callback objectives (LBFGS_OBJ_DEVICE), device-resident x0 / x, the canonical reductions on
caller-owned buffers (lbfgs_reducer_*) and their torch front end, on the GPU. Everything compares
bits. The cases themselves are in tests/devobj_gpu_cases.py:

1. the device callback against the oracle and the host-callback path, call counts included, also with
   line-search constants that are not the defaults;
2. real device math: torch objectives reduced through Reducer.sum, through LBFGS_OBJ_DEVICE and
   through LBFGS_OBJ_HOST, also on a non-default torch stream;
3. minimize_device / init_device / get_x_device against the host-buffer forms;
4. the refusals, a callback returning nonzero, a Python exception;
5. Reducer.dot / .sum against the oracle's canonical order and Context.dot.

Why a process of its own: a torch wheel brings its own copy of the HIP runtime, and zero-copy views
between torch and the library need both on ONE runtime. The library binds to torch's copy when torch
is imported before the library is loaded (same soname); the other order loads two runtimes and
torch then finds no GPU (lbfgs_amd raises a clear error for it). The rest of the suite loads the
library without torch and stays on the system runtime, so these cases run once, together, in a
child pytest that imports torch first; every test below reports one function of that run.
"""
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "devobj_gpu_cases.py")

# test function of the child run -> its number of cases
FUNCTIONS = {
    "test_device_callback_vs_oracle_and_host_path": 9,
    "test_device_callback_with_varied_constants": 24,
    "test_torch_objective_device_vs_host_route": 4,
    "test_torch_objective_on_a_side_stream": 1,
    "test_minimize_device_equals_minimize": 15,
    "test_init_device_step_get_x_device": 3,
    "test_host_objective_with_device_buffers": 1,
    "test_refusals": 1,
    "test_refused_on_a_sharded_context": 1,
    "test_callback_returning_nonzero_then_builtin": 1,
    "test_python_exception_is_reraised": 1,
    "test_reducer_vs_oracle_and_context_dot": 15,
    "test_reducer_rejects_other_tensors": 1,
}


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    xml = tmp_path_factory.mktemp("devobj") / "cases.xml"
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
