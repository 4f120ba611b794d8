"""AddressSanitizer + UBSan run of csrc/perm_diff.hpp, the host routine behind explain_permutations (and the host share of its
device form), as a stand-alone program (tests/sanitize/san_perm_diff.cpp includes that header alone): small matrices with every
buffer at its exact size -- the caps 0, 1 and the exact number of differing values, a pair whose values are all out of the
histogram's range, 512 rows, the list form.  Built here with g++ and run directly; no device, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_perm_diff_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_perm_diff")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Werror", "-I", os.path.join(ROOT, "starky_bn254_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "sanitize", "san_perm_diff.cpp")])
    r = subprocess.run([exe], env=SAN_ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out, err = r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")
    assert r.returncode == 0, (out[-2000:], err[-4000:])
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert "caps, out-of-range pairs, 512 rows and the list form ok" in out
