"""AddressSanitizer + UBSan run of csrc/witness_diff.hpp, the plain-C++ part of the witness diff (the tile compare, the statistics,
the row selection, the listing of a row, the launch cuts), as a stand-alone program (tests/sanitize/san_witness_diff.cpp includes
that header alone): 70 x 130 matrices, both dimensions ragged against the tile, at the caps 0, 1, exact and oversize, every buffer at
its exact size.  Built here with g++ and run directly; no device, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_witness_diff_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "san_witness_diff")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-Wall", "-Werror", "-I", os.path.join(ROOT, "starky_bn254_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "sanitize", "san_witness_diff.cpp")])
    r = subprocess.run([exe], env=SAN_ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out, err = r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")
    assert r.returncode == 0, (out[-2000:], err[-4000:])
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert "caps 0, 1, exact and oversize, and the launch cuts ok" in out
