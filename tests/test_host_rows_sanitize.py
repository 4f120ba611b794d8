"""AddressSanitizer + UBSan run of csrc/host_rows.hpp, the packing copy behind Prover.load_trace_rows, as a stand-alone program
(tests/sanitize/san_rows.cpp includes that header alone): every piece cut of a 7 x 5 matrix, from the flat form (packed and with a
stride of 8) and from the pointer form, every buffer at its exact size.  Built here with g++ and run directly; no device, nothing
loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_host_rows_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_rows")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Werror", "-I", os.path.join(ROOT, "starky_bn254_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "sanitize", "san_rows.cpp")])
    r = subprocess.run([exe], env=SAN_ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out, err = r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")
    assert r.returncode == 0, (out[-2000:], err[-4000:])
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert "piece cuts, both source forms and refusals ok" in out
