"""Aggregate check on the keyed group of a selector router without a device: the two-region slot layout of a call
(stylus_zkvm_verifiers_amd/csrc/zkv_gset_layout.h route_layout_agg) and the PREP lane's key lookup (zkv_gwset_prep.h gwset_key_of_slot2),
which tests/host_cpp/test_route_layout_agg.cpp checks against brute force over exhaustive small totals, every capable mask and every
sub-batch size, built plain and under the sanitizers and run as its own executable."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'host_cpp', 'test_route_layout_agg.cpp')
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']


@pytest.mark.parametrize('flags,name', [([], 'plain'), (SANITIZE, 'san')])
def test_route_layout_agg_equals_brute_force(tmp_path, flags, name):
    exe = str(tmp_path / name)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-Wno-unknown-pragmas'] + flags + ['-o', exe, SRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0 and not out.stderr, (out.returncode, out.stdout.decode()[-2000:], out.stderr.decode()[-2000:])
    word, count = out.stdout.decode().split()
    assert word == 'ok' and int(count) > 100000       # 4 sub-batch sizes x 6 totals per keyed column x every mask: 160 thousand layouts
