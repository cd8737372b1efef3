"""The plugin's ragged store path (host/tests/test_ragged.cc): a batch of
several shard sizes encoded by one memo_ec_encode_ragged call per staged
chunk, every block at its own shard size ("ragged-store"), and
Codec::encode_ragged / verify_ragged.  CPU: build + the device partition,
the shard offset arithmetic and the seeded batch's chunks.  GPU: mixed
stores with the key on and off, a uniform batch, the batcher and the codec
calls, RS(10,4) on 16 in-process nodes."""
import os
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "host")
BIN = os.path.join(HOST, "_build", "test_ragged")


def _build():
    subprocess.check_call(["make", "-s", "-j4", "-C", HOST])
    assert os.path.exists(BIN)


def _run(*args, timeout=300):
    r = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-4000:], r.stderr[-4000:])
    return r


def test_ragged_builds_and_cpu_tests_pass():
    _build()
    r = _run("--cpu-only")
    assert r.returncode == 0, r.stderr
    assert "3 tests, 0 failed" in r.stdout


def test_null_codec_defines_what_the_plugin_calls():
    """The GPU-free profiling build (make hostprof) links the plugin against
    the null codec: every memo_ec_* symbol the plugin's object needs must be
    defined there, the two ragged ones (null_codec_ragged.cc) among them."""
    _build()
    lib = os.path.join("_build", "hostprof", "libmemo_ec.so")
    subprocess.check_call(["make", "-s", "-C", HOST, lib])

    def symbols(flag, path):
        out = subprocess.run(["nm"] + flag.split() + [path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in out.splitlines() if "memo_ec_" in ln}

    need = symbols("-u", os.path.join(HOST, "_build", "erasure_consensus.o"))
    have = symbols("-D --defined-only", os.path.join(HOST, lib))
    assert {"memo_ec_encode_ragged", "memo_ec_verify_ragged"} <= need
    assert need <= have, sorted(need - have)


@pytest.mark.gpu
def test_ragged_store_on_gpu():
    _build()
    r = _run()
    assert r.returncode == 0, r.stdout + r.stderr
    assert "8 tests, 0 failed" in r.stdout
