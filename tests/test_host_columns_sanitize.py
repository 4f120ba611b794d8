"""AddressSanitizer + UBSan run of csrc/host_columns.hpp, the gather behind Prover.prove_host_columns, as a stand-alone program
(tests/sanitize/san_columns.cpp includes that header alone): every (word0, len) of a 5 x 8 matrix held as separate allocations,
every buffer at its exact size.  Built here with g++ and run directly; no device, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_host_columns_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_columns")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Werror", "-I", os.path.join(ROOT, "starky_bn254_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "sanitize", "san_columns.cpp")])
    r = subprocess.run([exe], env=SAN_ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out, err = r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")
    assert r.returncode == 0, (out[-2000:], err[-4000:])
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert "gather sweep and reduction ok" in out
