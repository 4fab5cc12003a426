"""The batched solver with a caller's objective for the whole batch (lbfgs_batch_set_device_objective,
Batch.set_device_objective), on the GPU. Everything compares bits. The cases themselves are in
tests/batchcb_gpu_cases.py:

1. against the single-problem path (LBFGS_OBJ_DEVICE with LBFGS_DEVICE_EAGER_GRAD) and the oracle;
2. rounds: as many calls as the largest f_calls, each problem active in exactly its first f_calls;
3. inactive rows are not read;
4. launch shape;
5. real device math: torch objectives per row, host and device forms, a non-default torch stream;
6. the guard paths: not-descent fallback, skipped updates, a failed line search;
7. refusals, a callback returning nonzero, a Python exception, clearing, the other objectives;
8. a history of 16 pairs and of 8, filled and rotated;
9. the size limit, n = 32768;
10. line-search constants that are not the defaults, and one row alone in a search of hundreds of rounds.

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
CASES = os.path.join(ROOT, "tests", "batchcb_gpu_cases.py")

# test function of the child run -> its number of cases
FUNCTIONS = {
    "test_inputs_exercise_the_paths": 1,
    "test_batch_callback_vs_single_path_and_oracle": 64,
    "test_rounds": 2,
    "test_a_problem_at_the_minimiser_is_active_once": 1,
    "test_inactive_rows_are_not_read": 3,
    "test_launch_shape_does_not_matter": 1,
    "test_torch_objective_batch_vs_single": 4,
    "test_guard_paths": 6,
    "test_guard_inputs_reach_the_guards": 1,
    "test_device_with_nothing_set_is_refused": 1,
    "test_refusals_and_clearing": 1,
    "test_callback_returning_nonzero_then_the_batch_goes_on": 1,
    "test_python_exception_is_reraised": 1,
    "test_other_objectives_of_the_batch_are_undisturbed": 1,
    "test_long_history": 20,
    "test_size_limit": 1,
    "test_varied_constants": 52,
    "test_one_row_alone_in_a_long_search": 1,
}


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    xml = tmp_path_factory.mktemp("batchcb") / "cases.xml"
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
