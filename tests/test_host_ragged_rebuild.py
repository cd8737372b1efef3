"""The plugin's ragged rebuild path (host/tests/test_ragged_rebuild.cc): a
staged chunk of several shard sizes rebuilt by one memo_ec_rebuild_ragged
call per erasure count and one per shared pattern, every survivor at its own
shard size ("ragged-rebuild"), and Codec::rebuild_ragged.  CPU: build + the
grouping, the staging's offset arithmetic and the device partition.  GPU: a
multi-address fetch with m holders down with the key on and off, a repair
after an eviction, a uniform-size batch and the codec call, RS(10,4) on 16
in-process nodes."""
import os
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "host")
BIN = os.path.join(HOST, "_build", "test_ragged_rebuild")


def _build():
    subprocess.check_call(["make", "-s", "-j4", "-C", HOST])
    assert os.path.exists(BIN)


def _run(*args, timeout=300):
    r = subprocess.run([BIN, *args], capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-4000:], r.stderr[-4000:])
    return r


def test_ragged_rebuild_builds_and_cpu_tests_pass():
    _build()
    r = _run("--cpu-only")
    assert r.returncode == 0, r.stderr
    assert "3 tests, 0 failed" in r.stdout


def test_null_codec_defines_the_ragged_rebuild():
    """The GPU-free profiling build (make hostprof) links the plugin against
    the null codec: every memo_ec_* symbol the plugin's object needs must be
    defined there, memo_ec_rebuild_ragged (null_codec_ragged_rebuild.cc)
    among them."""
    _build()
    lib = os.path.join("_build", "hostprof", "libmemo_ec.so")
    subprocess.check_call(["make", "-s", "-C", HOST, lib])

    def symbols(flag, path):
        out = subprocess.run(["nm"] + flag.split() + [path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in out.splitlines() if "memo_ec_" in ln}

    need = symbols("-u", os.path.join(HOST, "_build", "erasure_consensus.o"))
    have = symbols("-D --defined-only", os.path.join(HOST, lib))
    assert "memo_ec_rebuild_ragged" in need
    assert need <= have, sorted(need - have)


@pytest.mark.gpu
def test_ragged_rebuild_on_gpu():
    _build()
    r = _run()
    assert r.returncode == 0, r.stdout + r.stderr
    assert "7 tests, 0 failed" in r.stdout
