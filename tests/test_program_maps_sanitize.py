"""AddressSanitizer + UBSan run of the mapped links of the field programs on the host pool (csrc/program.hip on instance_lists.hpp)
as a stand-alone program: tests/sanitize/san_program_maps.cpp is compiled together with the host units that derivation calls, host
code instrumented, device code compiled uninstrumented and never launched.  The two Fq12 tables and FQ_EXP's refusal, num_io = 4,
every buffer at its exact size: the mapped derivation, the pad of a mapped last node, null optional outputs, the check and its
rejections, the refusals, sbn_fq12_frobenius and sbn_fq12_inverse.  Built here and run directly; no device, nothing loaded into
Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "starky_bn254_amd", "csrc")
UNITS = ["program.hip", "msm.hip", "msm_batch.hip", "scalar_mul.hip", "chain_instances.hip", "tracegen.hip"]
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_mapped_programs_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_program_maps")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                           "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-Wno-unused-variable",
                           "-o", exe] + [os.path.join(CSRC, u) for u in UNITS] + [os.path.join(ROOT, "tests", "sanitize", "san_program_maps.cpp")],
                          cwd=str(tmp_path))
    r = subprocess.run([exe], env=SAN_ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out, err = r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")
    assert r.returncode == 0, (out[-2000:], err[-4000:])
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert "the maps, the inverse, the schedule, mapped links, pads, optional outputs, the check's rejections and the refusals ok" in out
