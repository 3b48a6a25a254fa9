"""The resident resolver's 32-bit keys (custom-k8s-scheduler_amd/csrc/qs_key32.hpp), swept on the CPU.

tests/native/key32_sweep.cpp includes the header the kernels include and checks it against the 64-bit
key format pack_key(tv, node): for every tv in [0, 1024) and the nodes {0, 1, 2, 2^21 - 1, 2^21 + 1,
2^22 - 2, 2^22 - 1}, plus 1 M random pairs, convert(pack_key) == pack32, expand(pack32) == pack_key,
a64 < b64 <=> a32 < b32, and 0 <-> 0.  The GPU cases are in tests/test_gpu_resolver_k32.py.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("key32") / "key32_sweep")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", out,
                    os.path.join(HERE, "native", "key32_sweep.cpp")], check=True)
    return out


def test_key32_matches_the_64_bit_keys(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout
