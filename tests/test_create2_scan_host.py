"""vgen_scan_create2 on the CPU: scanner.cpp and cabi.cpp linked against the CPU stand-in of the runtime with CREATE2 contexts added
(tests/native/create2_rt.cpp: the single-source twin of the device block on the message words the kernel forms), built as a stand-alone
program with AddressSanitizer + UBSan.  tests/native/create2_driver.cpp holds every scan against a walk of the same counters with
vgen_create2_address: ascending counter order over one and several contexts, count cuts, max_batches per context, rings that
overflow, an on-device automaton, host filtering from dumps, the end of the counter space, and the refusals."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "vgen_amd", "csrc")
HOST = ["host_ec.cpp", "encode.cpp", "regex_dfa.cpp", "filter.cpp", "pattern_info.cpp", "provider.cpp"]


def test_scan_loop_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "create2_driver_asan")
    srcs = [os.path.join(NATIVE, "create2_driver.cpp"), os.path.join(NATIVE, "create2_rt.cpp"), os.path.join(CSRC, "scanner.cpp"), os.path.join(CSRC, "cabi.cpp")]
    srcs += [os.path.join(CSRC, "host", s) for s in HOST]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe] + srcs + ["-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("all ok"), r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert r.stdout.count("matches") == 8 and "complete 1" in r.stdout
