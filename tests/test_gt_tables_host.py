"""Fixed-base GT tables (csrc/zkv_gt.h), host side: the signed 20-bit recoding and the table indexing against Python integers, through
a stand-alone program that is also built and run under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import random
import subprocess

import pytest

import spec_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host_cpp', 'test_gt_recode.cpp')
W = 20


def signals():
    rng = random.Random(20)
    run = sum(((1 << 19) + 5) << (W * j) for j in range(12))          # every window hands a carry to the next
    ones = (1 << 253) - 1
    edge = [0, 1, (1 << 19) - 1, 1 << 19, (1 << 19) + 1, (1 << 20) - 1, 1 << 20, run, ones, m.R - 1, m.R - 2, (1 << 128) - 1, (1 << 253) - 1,
            (1 << 19) << W, ((1 << 20) - 1) << (W * 11)]
    return edge + [rng.randrange(m.R) for _ in range(200)] + [rng.randrange(1 << 128) for _ in range(50)]


def run_program(tmp_path, flags, name):
    exe = str(tmp_path / name)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g'] + flags + ['-o', exe, SRC])
    sig = signals()
    out = subprocess.run([exe], input=''.join('%064x\n' % s for s in sig).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert not out.stderr, out.stderr.decode()[-2000:]
    lines = out.stdout.decode().splitlines()
    assert lines[-1] == 'windows 7 13 13'
    return sig, [[tuple(int(x) for x in t.split(':')) for t in ln.split()] for ln in lines[:-1]]


@pytest.mark.parametrize('flags,name', [([], 'plain'), (['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], 'san')])
def test_recoding_and_indexing(tmp_path, flags, name):
    sig, rows = run_program(tmp_path, flags, name)
    assert len(rows) == len(sig)
    for s, row in zip(sig, rows):
        assert len(row) == 13
        digits = [d for d, _, _ in row]
        assert sum(d << (W * j) for j, d in enumerate(digits)) == s, hex(s)
        assert all(abs(d) <= 1 << 19 for d in digits), hex(s)
        if s < 1 << 128:
            assert not any(digits[7:]), hex(s)                       # a 128-bit signal ends within seven windows
        # the carry chain of the definition: d = window + carry in, minus 2^20 with a carry out when the window's top bit is set
        c = 0
        for j, d in enumerate(digits):
            w = (s >> (W * j)) & ((1 << W) - 1)
            assert d == w + c - ((w >> 19) << W), (hex(s), j)
            c = w >> 19
        assert c == 0
        for j, (d, row_word, off) in enumerate(row):
            assert row_word == j * (1 << 19) * 96
            assert off == ((abs(d) - 1) * 384 if d else 0)
            assert off + 384 <= (1 << 19) * 384 < 1 << 32            # inside the window's sub-table, below the 32-bit lane offset
