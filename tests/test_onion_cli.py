"""The command line and the onion format (format 13) without a device: `-f onion` is taken by generate and estimate and gets as far as
the device, the options that are no-ops are accepted, what the format cannot do is refused with a message before any device is opened,
and the stand-alone sanitizer build of the format's host code (tests/native/onion_selftest.cpp) exits 0.  (The outputs of a search -
text, jsonl, --key-dir - are checked on the GPU: tests/test_gpu_onion.py.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vgen_amd", "vgen-hip")
GOOD = ["generate", "-f", "onion", "-p", "^cat"]


def cli(*args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([CLI, *args], capture_output=True, text=True, env=env, timeout=60)


def test_the_format_is_named_and_gets_to_the_device(tmp_path):
    r = cli("generate", "-f", "nonsense", "-p", "^ca")
    assert r.returncode == 1 and "onion" in [x.strip(" )\n") for x in r.stderr.split("(", 1)[1].split(",")]
    for extra in ([], ["-i", "-c", "3", "-o", "jsonl", "--devices", "0", "--seed", "7"], ["--random-keys"], ["--no-endo"],
                  ["--key-dir", str(tmp_path)], ["-o", "csv", "--file", str(tmp_path / "out.csv")]):
        r = cli(*GOOD, *extra)
        assert r.returncode == 1 and "no HIP device" in r.stderr, (extra, r.stderr)
    r = cli("estimate", "-f", "onion", "-p", "^cat")
    assert r.returncode == 1 and "no HIP device" in r.stderr and "--format" not in r.stderr, r.stderr
    r = cli("--help")
    assert "-f onion" in r.stderr and "--key-dir" in r.stderr and "NEIGHBOURS" in r.stderr


def test_invalid_characters_are_warned_about():
    r = cli("generate", "-f", "onion", "-p", "^c0t8")
    assert "not valid in Base32" in r.stderr and "'08'" in r.stderr


@pytest.mark.parametrize("args,word", [
    (["range", "-f", "onion", "--puzzle", "20"], "range"),
    (["range", "-f", "onion", "--range", "1:ff", "-p", "^ca"], "range"),
    (GOOD + ["--checkpoint", "/tmp/never-written.ck"], "--checkpoint"),
    (["generate", "-f", "onion", "--patterns-file", "/dev/null"], "--patterns-file"),
    (GOOD + ["--base-pubkey", "0279be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798"], "--base-pubkey"),
    (["generate", "-f", "onion", "-p", "score:zero-bytes>=2"], "score"),
    (["verify", "-f", "onion"], "verify"),
])
def test_refusals_come_with_a_message_and_before_the_device(args, word):
    r = cli(*args)
    assert r.returncode == 1 and "no HIP device" not in r.stderr and word in r.stderr and "Error:" in r.stderr, r.stderr


def test_the_key_directory_belongs_to_the_format(tmp_path):
    r = cli("generate", "-f", "p2pkh", "-p", "^1A", "--key-dir", str(tmp_path))
    assert r.returncode == 1 and "--key-dir" in r.stderr and "no HIP device" not in r.stderr


def test_the_sanitizer_selftest_passes():
    exe = os.path.join(ROOT, "tests", "native", "onion_selftest")
    assert os.path.exists(exe), f"{exe} not built (make -C tests/native -f onion.mk, or __graft_entry__.build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
