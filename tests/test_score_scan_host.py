"""Score searches through the scan loops on the CPU: scanner.cpp and cabi.cpp linked against the CPU stand-in of the runtime with score
filters added (tests/native/score_rt.cpp: the stand-in and its CREATE2 contexts as they are, the candidates scored with the
single-source core/score_eval.h against the terms each dispatch was enqueued with), built as a stand-alone program with
AddressSanitizer + UBSan.  tests/native/score_driver.cpp holds every scan against a walk of the same counters / keys: a threshold
scan equals the walk, VGEN_SCAN_BEST equals its running maximum over one context and over several, `count` cuts both (a plain count cut
over several contexts keeps whichever hits its contexts reach first: any `count` of the walk's, in key order),
vgen_set_score_min changes later dispatches only, and the refusals hold."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "vgen_amd", "csrc")
HOST = ["host_ec.cpp", "encode.cpp", "regex_dfa.cpp", "filter.cpp", "pattern_info.cpp", "provider.cpp"]


def test_score_scans_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "score_driver_asan")
    srcs = [os.path.join(NATIVE, "score_driver.cpp"), os.path.join(NATIVE, "score_rt.cpp"), os.path.join(CSRC, "scanner.cpp"), os.path.join(CSRC, "cabi.cpp")]
    srcs += [os.path.join(CSRC, "host", s) for s in HOST]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-parameter", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe] + srcs + ["-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("all ok"), r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert r.stdout.count(" results, ") == 16 and r.stdout.count(" best ") == 9
