"""vgen_scan_create3 on the CPU: scanner.cpp and cabi.cpp linked against the CPU stand-in of the runtime with CREATE3 jobs added
(tests/native/create3_rt.cpp: the single-source twins of the device blocks on the message words the kernels form), built as a
stand-alone program with AddressSanitizer + UBSan.  tests/native/create3_driver.cpp holds every scan against a plain walk of the
same counters with vgen_create3_address: regex and score patterns, VGEN_SCAN_BEST, count cuts, max_batches per context, one and two
contexts, rings that overflow, an on-device automaton, host filtering from dumps, the end of the counter space, the refusals, and a
CREATE2 scan on contexts a CREATE3 scan used before.  Nothing here is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "vgen_amd", "csrc")
HOST = ["host_ec.cpp", "encode.cpp", "regex_dfa.cpp", "filter.cpp", "pattern_info.cpp", "provider.cpp"]


def test_scan_loop_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "create3_driver_asan")
    srcs = [os.path.join(NATIVE, "create3_driver.cpp"), os.path.join(NATIVE, "create3_rt.cpp"), os.path.join(CSRC, "scanner.cpp"), os.path.join(CSRC, "cabi.cpp")]
    srcs += [os.path.join(CSRC, "host", s) for s in HOST]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe] + srcs + ["-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("all ok"), r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert "cases 14" in r.stdout and r.stdout.count("complete 1") == 1
    assert "round 0 (create3)" in r.stdout and "round 1 (create2)" in r.stdout and "round 2 (create3)" in r.stdout
