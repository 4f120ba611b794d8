"""examples/c/prove_host_trace: the host-trace call and the cached one-shot call from compiled C (no Python in the process that
proves).  It must print the checksum of the proof the Python binding gets for the same instance list."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_c_examples import EX, _checksum


def test_c_example_host_trace_builds_against_the_header():
    subprocess.check_call(["make", "-s", "-C", EX, "prove_host_trace"])
    assert os.path.exists(os.path.join(EX, "prove_host_trace"))


@pytest.mark.gpu
def test_c_example_host_trace_proves_the_same_proof(S, O, tmp_path):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device")
    subprocess.check_call(["make", "-s", "-C", EX])
    ios, _ = O.g1exp_inputs(128, 1)
    np.ascontiguousarray(ios, dtype="<u4").tofile(tmp_path / "g1.bin")
    out = subprocess.run([os.path.join(EX, "prove_host_trace"), str(tmp_path / "g1.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode()
    assert out.returncode == 0 and "verified" in text and "1 hit, 1 miss" in text, text
    stark = S.G1ExpStark(128)
    p = S.Prover(stark, stark.config(), 16)
    p.generate_trace(ios)
    want = _checksum(p.prove().words)
    p.close()
    assert re.search(r"checksum ([0-9a-f]{16})", text).group(1) == want, text
