"""The command line and the Solana format (format 12) without a device: `-f solana` is taken by generate and estimate and gets as far as
the device, the options that are no-ops are accepted, and what the format cannot do is refused with a message before any device is
opened.  (The outputs of a search - text, json, --keypair-dir - are checked on the GPU: tests/test_gpu_solana.py.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "vgen_amd", "vgen-hip")
GOOD = ["generate", "-f", "solana", "-p", "^So1"]


def cli(*args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([CLI, *args], capture_output=True, text=True, env=env, timeout=60)


def test_the_format_is_named_and_gets_to_the_device(tmp_path):
    r = cli("generate", "-f", "nonsense", "-p", "^So")
    assert r.returncode == 1 and "solana" in [x.strip(" )\n") for x in r.stderr.split("(", 1)[1].split(",")]
    for extra in ([], ["-i", "-c", "3", "-o", "jsonl", "--devices", "0", "--seed", "7"], ["--random-keys"], ["--no-endo"],
                  ["--keypair-dir", str(tmp_path)], ["-o", "csv", "--file", str(tmp_path / "out.csv")]):
        r = cli(*GOOD, *extra)
        assert r.returncode == 1 and "no HIP device" in r.stderr, (extra, r.stderr)
    r = cli("estimate", "-f", "solana", "-p", "^So1")
    assert r.returncode == 1 and "no HIP device" in r.stderr and "--format" not in r.stderr, r.stderr
    r = cli("--help")
    assert "-f solana" in r.stderr and "--keypair-dir" in r.stderr


def test_invalid_characters_are_warned_about():
    r = cli("generate", "-f", "solana", "-p", "^S0l")
    assert "not valid in Base58" in r.stderr and "'0l'" in r.stderr


@pytest.mark.parametrize("args,word", [
    (["range", "-f", "solana", "--puzzle", "20"], "range"),
    (["range", "-f", "solana", "--range", "1:ff", "-p", "^So"], "range"),
    (GOOD + ["--checkpoint", "/tmp/never-written.ck"], "--checkpoint"),
    (["generate", "-f", "solana", "--patterns-file", "/dev/null"], "--patterns-file"),
    (GOOD + ["--base-pubkey", "0279be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798"], "--base-pubkey"),
    (["generate", "-f", "solana", "-p", "score:zero-bytes>=2"], "score"),
])
def test_refusals_come_with_a_message_and_before_the_device(args, word):
    r = cli(*args)
    assert r.returncode == 1 and "no HIP device" not in r.stderr and word in r.stderr and "Error:" in r.stderr, r.stderr


def test_the_keypair_directory_belongs_to_the_format(tmp_path):
    r = cli("generate", "-f", "p2pkh", "-p", "^1A", "--keypair-dir", str(tmp_path))
    assert r.returncode == 1 and "--keypair-dir" in r.stderr and "no HIP device" not in r.stderr
