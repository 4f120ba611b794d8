"""Host replay of tests/golden/instance_list_refusals.json (no device): every recorded call of the five instance-list units
(chained lists, long MSMs, scalar multiplications, field powers, segmented batches) is made again on the library under test, and
its return code, its full sbn_last_error() text and the SHA-256 of every output array must equal the record.  The record was
taken before the units were folded onto one shared header (tests/golden/make_instance_list_refusals.py says how, and which
refusals no call can reach); the inputs are rebuilt by that file's builders from Python integers."""
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENTRY_POINTS = {"sbn_chain_instances", "sbn_msm_instances", "sbn_msm_check_links", "sbn_scalar_mul_instances", "sbn_scalar_mul_check", "sbn_mul_by_cofactor_check",
                "sbn_power_instances", "sbn_power_check", "sbn_msm_batch_instances", "sbn_msm_batch_check", "sbn_curve_generator", "sbn_g2_cofactor", "sbn_bn_x"}


def _maker():
    spec = importlib.util.spec_from_file_location("make_instance_list_refusals", os.path.join(GOLDEN, "make_instance_list_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_recorded_case_replays(S):
    M = _maker()
    with open(os.path.join(GOLDEN, "instance_list_refusals.json")) as f:
        cases = json.load(f)
    assert {c["call"] for c in cases} == ENTRY_POINTS
    assert [(c["call"], c["builder"], c["params"]) for c in cases] == [(c["call"], c["builder"], c["params"]) for c, _ in M._cases()], "the record is not the generator's case list"
    differ = []
    for i, case in enumerate(cases):
        rc, text, digests = M.run_case(S.lib(), case)
        if (rc, text, digests) != (case["rc"], case["error"], case["sha256"]):
            differ.append((i, case["call"], case["params"], (rc, text), (case["rc"], case["error"])))
    assert not differ, (len(differ), differ[:5])
