"""Slot and record layout of a selector-router call (stylus_zkvm_verifiers_amd/csrc/zkv_gset_layout.h route_layout: the SP1 gateway's and
the RISC Zero router's one layout function) without a device: tests/host_cpp/test_route_layout.cpp checks it against brute force over
exhaustive small and seeded random column totals, built plain and under the sanitizers and run as its own executable."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'host_cpp', 'test_route_layout.cpp')
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']


@pytest.mark.parametrize('flags,name', [([], 'plain'), (SANITIZE, 'san')])
def test_route_layout_equals_brute_force(tmp_path, flags, name):
    exe = str(tmp_path / name)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror'] + flags + ['-o', exe, SRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0 and not out.stderr, (out.returncode, out.stdout.decode()[-2000:], out.stderr.decode()[-2000:])
    word, count = out.stdout.decode().split()
    assert word == 'ok' and int(count) > 100000       # the exhaustive shapes alone are several hundred thousand layouts
