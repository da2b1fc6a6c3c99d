"""CPU counterpart of tests/test_device_primitives_gpu.py: the same case generators and references (tests/primitive_cases.py) through
host builds of the same harness (stylus_zkvm_verifiers_amd/csrc/zkv_selftest.h compiled by tests/host_sim/host_sim_selftest*.cpp, lanes
played by threads), so that the generators, the reference conversions and the harness are checked before any GPU time is spent; and
the argument checks of zkv_diag_primitive, which happen before any launch."""
import ctypes as C

import numpy as np
import pytest

import primitive_cases as pc


@pytest.mark.parametrize('op,n', [(0, 600), (1, 600), (2, 300), (3, 300), (4, 600), (5, 300), (6, 300), (7, 200)])
def test_lane_ops_on_the_host_build(op, n):
    ins = pc.cases_for(0, op, n, 7)
    pc.check(0, op, ins, pc.run_host(0, op, ins))


@pytest.mark.parametrize('mapping,op,n', [(1, 0, 200), (1, 1, 600), (1, 2, 300), (1, 3, 9), (1, 4, 9), (2, 0, 9), (2, 1, 9), (3, 0, 5), (3, 1, 5)])
def test_pair_and_wide_ops_on_the_host_build(mapping, op, n):
    ins = pc.cases_for(mapping, op, n, 7)
    pc.check(mapping, op, ins, pc.run_host(mapping, op, ins))


def test_references_agree_with_spec_model():
    """the shortcuts of the references: the linear Frobenius against f12pow(a, p^k), the slot <-> w-basis conversion round trip"""
    import random
    import spec_model as m
    rng = random.Random(3)
    a = [rng.randrange(m.P) for _ in range(12)]
    assert pc.slots_to_f12(pc.f12_to_slots(a)) == a
    for k in (1, 2, 3):
        assert pc.f12_frob(a, k) == m.f12pow(a, m.P ** k)
    c = pc.cyclotomic_pool()[0]
    assert m.f12mul(c, pc.f12_conj(c)) == m.F12_ONE           # cyclotomic: the conjugate is the inverse
    lam = m.g1_mul((1, 2), pc.GLV_LAMBDA)                       # the GLV endomorphism: lambda (x, y) = (beta x, y), beta^3 = 1
    assert lam[1] == 2 and lam[0] != 1 and pow(lam[0], 3, m.P) == 1


def test_header_declares_exactly_the_harness_symbols():
    """include/zkv_diag_primitive.h is a companion of zkv.h: its entry point is bound by diag_primitive.SYMBOLS, not _lib.SYMBOLS"""
    import os
    import re
    from stylus_zkvm_verifiers_amd import _lib, diag_primitive
    root = os.path.dirname(pc.HERE)
    hdr = open(os.path.join(root, 'include', 'zkv_diag_primitive.h')).read()
    declared = set(re.findall(r'\b(zkv_\w+)\s*\(', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)))
    assert declared == set(diag_primitive.SYMBOLS) == {'zkv_diag_primitive'}
    assert '#include "zkv.h"' in hdr and '#define ZKV_DIAG_PRIMITIVE_MAX_CASES %d' % diag_primitive.MAX_CASES in hdr
    zkv_h = open(os.path.join(root, 'include', 'zkv.h')).read()
    for s in declared:
        assert s not in zkv_h and s not in _lib.SYMBOLS, s
    L = diag_primitive.lib()                  # binds every symbol: AttributeError if one is not exported
    assert all(hasattr(L, s) for s in declared)


def test_diag_primitive_argument_checks():
    from stylus_zkvm_verifiers_amd import _lib, diag_primitive
    L = diag_primitive.lib()
    buf = np.zeros(4096, dtype=np.uint32)
    p = buf.ctypes.data_as(C.POINTER(C.c_uint32))
    for mapping, op, n in ((0, 8, 1), (0, -1, 1), (1, 5, 1), (2, 2, 1), (3, 2, 1), (4, 0, 1), (-1, 0, 1), (0, 0, 0), (1, 3, 0), (0, 0, diag_primitive.MAX_CASES + 1)):
        assert L.zkv_diag_primitive(0, mapping, op, n, p, p) == _lib.ERR_INVALID_ARG, (mapping, op, n)
    assert L.zkv_diag_primitive(0, 0, 0, 1, None, p) == _lib.ERR_INVALID_ARG
    for dev in (-1, 99):                       # no such device (on a machine without a GPU every index is one)
        assert L.zkv_diag_primitive(dev, 0, 0, 1, p, p) == _lib.ERR_NO_DEVICE
