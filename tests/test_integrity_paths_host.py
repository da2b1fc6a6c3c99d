"""verify_integrity on every batch path (device-resident, verifier sets, mixed batches with a per-proof method): what holds without a
GPU -- the five entry points are exported, argument errors come back before the device is touched, and the numpy model of the
extended partition (tests/mixed_model.py, reused by tests/test_integrity_paths_gpu.py) follows the rules of include/zkv.h."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import mixed_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = bytes.fromhex
NEW = ['zkv_risc0_verify_integrity_batch_dev', 'zkv_risc0_set_verify_integrity_batch', 'zkv_risc0_set_verify_integrity_batch_dev',
       'zkv_mixed_verify_call_batch', 'zkv_mixed_verify_call_batch_dev']


@pytest.fixture(scope='module')
def L():
    from stylus_zkvm_verifiers_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_new_entry_points_are_declared_and_exported(L):
    from stylus_zkvm_verifiers_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'zkv.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(zkv_[a-z0-9_]+)\s*\(', hdr))
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(raw, name), name
    assert declared == set(_lib.SYMBOLS) and len(declared) == 78 + len(NEW)       # 78 before these five
    assert re.search(r'#define ZKV_METHOD_VERIFY 0\b', hdr) and re.search(r'#define ZKV_METHOD_VERIFY_INTEGRITY 1\b', hdr)


def _contexts(L, real_proofs):
    r = real_proofs['risc0']
    pk = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'plonk_cases.json')))
    pkvk = H(pk['vk'])
    ctx = {
        'risc0': L.zkv_risc0_ctx_create(H(r['control_root']), H(r['bn254_control_id']), 0),
        'risc0_new': L.zkv_risc0_ctx_new(0),
        'set': L.zkv_risc0_set_create(2, H(r['control_root']) * 2, H(r['bn254_control_id']) * 2, 0),
        'sp1': L.zkv_sp1_ctx_create(0),
        'plonk': L.zkv_sp1_plonk_ctx_create(pkvk, len(pkvk), H(pk['verifier_hash']), 0),
        'groth16': L.zkv_groth16_ctx_create(bytes(448 + 64 * 3), 3, 1, 0),
        'mixed': L.zkv_mixed_ctx_create(H(r['control_root']), H(r['bn254_control_id']), 0),
    }
    assert all(ctx.values()), ctx
    return ctx


def test_argument_errors_need_no_device(L, real_proofs):
    from stylus_zkvm_verifiers_amd import _lib
    ctx = _contexts(L, real_proofs)
    OK, ARG, WRONG = _lib.OK, _lib.ERR_INVALID_ARG, _lib.ERR_WRONG_CTX
    p = 1                                                               # a non-null "device pointer": never dereferenced on these paths
    buf = np.zeros(4096, dtype=np.uint8); b = buf.ctypes.data
    off = np.array([0, 260, 520], dtype=np.uint64); o = off.ctypes.data
    inst = np.zeros(2, dtype=np.uint32); ip = inst.ctypes.data
    r0_dev = lambda h, n, *a: L.zkv_risc0_verify_integrity_batch_dev(h, n, *a)
    set_h = lambda h, n, *a: L.zkv_risc0_set_verify_integrity_batch(h, n, *a)
    set_d = lambda h, n, *a: L.zkv_risc0_set_verify_integrity_batch_dev(h, n, *a)
    mix_h = lambda h, n, *a: L.zkv_mixed_verify_call_batch(h, n, *a)
    mix_d = lambda h, n, *a: L.zkv_mixed_verify_call_batch_dev(h, n, *a)
    # the wrong kind of context, whatever the other arguments
    for k in ('sp1', 'plonk', 'groth16', 'set', 'mixed', None):
        h = ctx[k] if k else None
        assert r0_dev(h, 2, p, p, p, None, None) == WRONG, k
    for k in ('risc0', 'risc0_new', 'sp1', 'plonk', 'groth16', 'mixed', None):
        h = ctx[k] if k else None
        assert set_h(h, 2, ip, b, o, b, b, None) == WRONG, k
        assert set_d(h, 2, p, p, p, p, None, None) == WRONG, k
    for k in ('risc0', 'set', 'sp1', 'plonk', 'groth16', None):
        h = ctx[k] if k else None
        assert mix_h(h, 2, b, b, b, o, b, b, o, b, None) == WRONG, k
        assert mix_d(h, 2, p, p, p, p, p, 32, 0, p, None, None) == WRONG, k
    # NULL required pointers with n > 0
    assert r0_dev(ctx['risc0'], 2, None, p, p, None, None) == ARG
    assert r0_dev(ctx['risc0'], 2, p, None, p, None, None) == ARG
    assert r0_dev(ctx['risc0'], 2, p, p, None, None, None) == ARG
    assert r0_dev(ctx['risc0_new'], 2, p, None, p, None, None) == ARG      # before the un-initialised answer, which needs the device
    for i in range(5):
        a = [ip, b, o, b, b]; a[i] = None
        assert set_h(ctx['set'], 2, *a, None) == ARG, i
    for i in range(5):
        a = [p, p, p, p]; a[min(i, 3)] = None
        if i < 4:
            assert set_d(ctx['set'], 2, *a, None, None) == ARG, i
    for i in (0, 2, 3, 4, 5, 6, 7, 8):                                   # method (1) and recv may be NULL
        a = [b, b, b, o, b, b, o, b]; a[i - 1 if i else 0] = None
        assert mix_h(ctx['mixed'], 2, *(a[:1] + [b] + a[1:]), None) == ARG, i
    for i in (0, 1, 2, 3, 4):
        a = [p, p, p, p, p]; a[i] = None                                     # vm, seals, in_a, in_b, status
        assert mix_d(ctx['mixed'], 2, a[0], p, a[1], a[2], a[3], 32, 0, a[4], None, None) == ARG, i
    assert mix_d(ctx['mixed'], 2, p, p, p, p, p, 16, 0, p, None, None) == ARG       # b_stride < 32
    assert mix_d(ctx['mixed'], 2, p, p, p, p, p, 96, 97, p, None, None) == ARG      # pv_len > b_stride
    # host call: a RISC Zero verify row's journal digest is exactly 32 bytes; an integrity row's in_b is not read (any length)
    vm = np.array([0, 0], dtype=np.uint8); meth = np.array([0, 1], dtype=np.uint8)
    call = lambda m, boff: mix_h(ctx['mixed'], 2, vm.ctypes.data, m, b, o, b, b, np.asarray(boff, dtype=np.uint64).ctypes.data, b, None)
    assert call(meth.ctypes.data, [0, 31, 31]) == ARG
    assert call(None, [0, 32, 40]) == ARG                                    # NULL method: both rows are verify rows
    assert call(meth.ctypes.data, [0, 64, 32]) == ARG                        # offsets run backwards
    # n = 0 with null pointers
    assert r0_dev(ctx['risc0'], 0, None, None, None, None, None) == OK
    assert set_h(ctx['set'], 0, None, None, None, None, None, None) == OK
    assert set_d(ctx['set'], 0, None, None, None, None, None, None) == OK
    assert mix_h(ctx['mixed'], 0, None, None, None, None, None, None, None, None, None) == OK
    assert mix_d(ctx['mixed'], 0, None, None, None, None, None, 0, 0, None, None, None) == OK
    import torch
    if not torch.cuda.is_available():                                      # the valid calls reach the device: no CPU fallback
        assert call(meth.ctypes.data, [0, 32, 32]) == _lib.ERR_NO_DEVICE
        assert call(meth.ctypes.data, [0, 32, 39]) == _lib.ERR_NO_DEVICE     # the integrity row's 7 bytes are fine
        assert set_h(ctx['set'], 2, ip, b, o, b, b, None) == _lib.ERR_NO_DEVICE
    for h in ctx.values():
        L.zkv_ctx_destroy(h)


def test_python_mirror_rejects_what_the_c_side_would_misread(L, real_proofs):
    import stylus_zkvm_verifiers_amd as z
    r = real_proofs['risc0']
    mx = z.MixedVerifier(H(r['control_root']), H(r['bn254_control_id']))
    with pytest.raises(ValueError):
        mx.verify_batch([0, 0], [b'', b''], [bytes(32)] * 2, [bytes(32)] * 2, methods=[1])
    with pytest.raises(ValueError):
        mx.verify_batch([0], [b''], [bytes(31)], [b''], methods=[1])
    s = z.RiscZeroVerifierSet([H(r['control_root'])], [H(r['bn254_control_id'])])
    with pytest.raises(ValueError):
        s.verify_integrity_batch([0, 0], [b''], [bytes(32)])
    st, rv = s.verify_integrity_batch([], [], [])
    assert len(st) == 0 and rv.shape == (0, 4)
    assert z.mixed.METHOD_VERIFY == 0 and z.mixed.METHOD_VERIFY_INTEGRITY == 1 and z.mixed.STATUS_BAD_CALLDATA == z.errors.STATUS_BAD_CALLDATA == 6


def test_partition_model_follows_the_rules():
    rng = np.random.default_rng(0x1A7E)
    for n in (1, 2, 255, 256, 257, 5000):
        vm, meth = mm.random_calls(rng, n, p_bad=0.1)
        idx, n0, kind, unplaced, st = mm.partition(vm, meth)
        # every proof exactly once: placed or answered in place
        assert sorted(np.concatenate([idx, unplaced]).tolist()) == list(range(n))
        # RISC Zero first, then SP1; stable within each
        assert (vm[idx[:n0]] == 0).all() and (vm[idx[n0:]] == 1).all()
        assert (np.diff(idx[:n0]) > 0).all() and (np.diff(idx[n0:]) > 0).all()
        # the compact RISC Zero method is the proof's, and only verify / verify_integrity get there; SP1 rows only with method 0
        assert (kind == meth[idx[:n0]]).all() and set(kind.tolist()) <= {0, 1}
        assert (meth[idx[n0:]] == 0).all()
        # unplaced: an unknown tag wins over the method; a method the VM lacks is BAD_CALLDATA
        want = np.where(vm[unplaced] > 1, mm.STATUS_UNKNOWN_VM, mm.STATUS_BAD_CALLDATA)
        assert (st == want).all()
        assert (((vm[unplaced] == 0) & (meth[unplaced] > 1)) | ((vm[unplaced] == 1) & (meth[unplaced] > 0)) | (vm[unplaced] > 1)).all()
    # pinned cases
    vm = np.array([0, 0, 1, 2, 0, 1, 1, 0, 2], dtype=np.uint8)
    me = np.array([0, 1, 0, 1, 2, 1, 0, 255, 0], dtype=np.uint8)
    idx, n0, kind, unplaced, st = mm.partition(vm, me)
    assert idx.tolist() == [0, 1, 2, 6] and n0 == 2 and kind.tolist() == [0, 1]
    assert unplaced.tolist() == [3, 4, 5, 7, 8] and st.tolist() == [7, 6, 6, 6, 7]
    # NULL method = all verify: the partition of the method-less call
    idx2, n02, kind2, unplaced2, st2 = mm.partition(vm)
    assert idx2.tolist() == [0, 1, 4, 7, 2, 5, 6] and n02 == 4 and (kind2 == 0).all() and st2.tolist() == [7, 7]
    # the mix random_calls draws
    vm, me = mm.random_calls(np.random.default_rng(1), 30000)
    c = mm.classify(vm, me)
    for v, m in ((0, 0), (0, 1), (1, 0)):
        assert 0.28 < ((vm == v) & (me == m)).mean() < 0.36, (v, m)
    assert 0 < (c == 2).sum() and 0 < (c == 3).sum()


def test_integrity_batches_from_the_real_proof(real_proofs):
    from stylus_zkvm_verifiers_amd import synth
    r = real_proofs['risc0']
    seals, claims, lens, mut, cls = synth.make_integrity_batch(H(r['seal']), H(r['claim_digest']), 300, 7, pool=2, mutate_every=5)
    assert seals.shape == (300, 260) and claims.shape == (300, 32) and mut.sum() == 60
    assert (seals[:, :4] == np.frombuffer(H(r['seal'])[:4], dtype=np.uint8)).all(axis=1).sum() == 300 - (cls == 1).sum()
    assert ((claims != np.frombuffer(H(r['claim_digest']), dtype=np.uint8)).any(axis=1) == (cls == 0)).all()
    assert ((lens < 260) == (cls == 2)).all() and (lens >= 4).all()
    assert set(cls[mut].tolist()) == {0, 1, 2} and (cls[~mut] == -1).all()
    assert len({seals[i].tobytes() for i in range(300)}) > 250            # re-randomised, not copies
