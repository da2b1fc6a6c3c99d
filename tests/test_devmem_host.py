"""The device-memory owners (stylus_zkvm_verifiers_amd/csrc/zkv_devmem.h) without a device: tests/host_cpp/test_devmem.cpp runs them over a
counting fake of the runtime that refuses on request -- growth policy, exact allocations, release and moves, the reset of an aggregate of
owners, a refusal at every position of a group of allocations -- built plain and under the sanitizers and run as its own executable."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'host_cpp', 'test_devmem.cpp')
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']


@pytest.mark.parametrize('flags,name', [([], 'plain'), (SANITIZE, 'san')])
def test_owners_against_counting_fake(tmp_path, flags, name):
    exe = str(tmp_path / name)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror'] + flags + ['-o', exe, SRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0 and not out.stderr, (out.returncode, out.stdout.decode()[-2000:], out.stderr.decode()[-2000:])
    word, count = out.stdout.decode().split()
    assert word == 'ok' and int(count) > 100
