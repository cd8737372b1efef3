"""ErasureConsensus::scrub() (host/tests/test_scrub.cc): every block's k + m
shards verified on the GPU, the wrong shard the code names rewritten, the
rest handed to the k-subset recovery.  CPU: build + the verdict decoding and
ScrubReport arithmetic.  GPU: every case, RS(10,4) on 16 in-process nodes."""
import os
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "host")
BIN = os.path.join(HOST, "_build", "test_scrub")


def _build():
    subprocess.check_call(["make", "-s", "-j4", "-C", HOST])
    assert os.path.exists(BIN)


def _run(*args, timeout=300):
    r = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-4000:], r.stderr[-4000:])
    return r


def test_scrub_builds_and_cpu_tests_pass():
    _build()
    r = _run("--cpu-only")
    assert r.returncode == 0, r.stderr
    assert "2 tests, 0 failed" in r.stdout


@pytest.mark.gpu
def test_scrub_on_gpu():
    _build()
    r = _run()
    assert r.returncode == 0, r.stdout + r.stderr
    assert "9 tests, 0 failed" in r.stdout
