"""AddressSanitizer + UBSan run of the curve programs on the host pool (csrc/curve_program.hip on instance_lists.hpp) as a
stand-alone program: tests/sanitize/san_curve_program.cpp is compiled together with the host units that derivation calls, host
code instrumented, device code compiled uninstrumented and never launched.  Both curve tables, num_io = 4, every buffer at its
exact size: every kind of operand, links across unit boundaries, the pads, a choice moved by a crafted literal, the values, null
optional outputs, the check's rejections, a program no candidate mends, the refusals.  Built here and run directly; no device,
nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "starky_bn254_amd", "csrc")
UNITS = ["curve_program.hip", "program.hip", "msm.hip", "msm_batch.hip", "scalar_mul.hip", "chain_instances.hip", "tracegen.hip"]
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_curve_programs_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_curve_program")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                           "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-Wno-unused-variable",
                           "-o", exe] + [os.path.join(CSRC, u) for u in UNITS] + [os.path.join(ROOT, "tests", "sanitize", "san_curve_program.cpp")],
                          cwd=str(tmp_path))
    r = subprocess.run([exe], env=SAN_ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out, err = r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")
    assert r.returncode == 0, (out[-2000:], err[-4000:])
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert "links, starts, pads, values, optional outputs, the check's rejections and the refusals ok" in out
