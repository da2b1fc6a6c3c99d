"""eth_call batches on a Groth16 key set of deployed contracts (include/zkv_groth16_set_wire.h) without a device: the
header against the library's exports, the selector strings against the model's (tests/groth16_set_wire_model.py), creation's refusals,
the seeded case list against the oracle alone, and the decode function the kernel runs (csrc/zkv_wire_gset.h, compiled for the host)
against the model on that list.  PARITY UNPINNED: the reference holds no generic contract shell."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import groth16_set_wire_model as gm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ['zkv_groth16_set_create_deployed', 'zkv_groth16_set_call_selector', 'zkv_groth16_set_eth_call_batch', 'zkv_groth16_set_eth_call_batch_dev',
       'zkv_groth16_set_eth_call_returndata', 'zkv_groth16_set_last_call_counts']
WRONG_CTX, INVALID_ARG = -5, -1


@pytest.fixture(scope='module')
def L():
    from stylus_zkvm_verifiers_amd import groth16_set_wire
    return groth16_set_wire.lib()


@pytest.fixture(scope='module')
def world():
    keys, tds = gm.deployed_set()
    reqs = gm.requests(keys, tds)
    model = gm.Contracts(keys)
    return keys, reqs, model, gm.expected(model, reqs)


@pytest.fixture(scope='module')
def hs():
    src = os.path.join(HERE, 'host_sim', 'host_sim_gset_wire.cpp')
    lib = os.path.join(HERE, 'host_sim', 'libhost_sim_gset_wire.so')
    csrc = os.path.join(ROOT, 'stylus_zkvm_verifiers_amd', 'csrc')
    deps = [src] + [os.path.join(csrc, f) for f in ('zkv_wire_gset.h', 'zkv_sha256.h', 'zkv_field.h')]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-Wno-unknown-pragmas', '-o', lib, src])
    S = C.CDLL(lib)
    S.hsgsw_decode.argtypes = [C.c_uint64, C.c_char_p, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 6 + [C.c_int]
    return S


def _names(path):
    return set(re.findall(r'\b(zkv_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)))


def _vk(n_ic):
    return bytes(448 + 64 * n_ic)


def _create(L, keys):
    k = len(keys)
    words = (C.c_char_p * k)(*[key[0] for key in keys])
    return L.zkv_groth16_set_create_deployed(k, words, (C.c_size_t * k)(*[key[1] for key in keys]), (C.c_int * k)(*[key[2] for key in keys]),
                                             b''.join(key[3] for key in keys), bytes(key[4] for key in keys), 0)


def test_header_declares_the_new_symbols_and_the_library_exports_them(L):
    hdr = os.path.join(ROOT, 'include', 'zkv_groth16_set_wire.h')
    assert _names(hdr) == set(NEW)
    text = open(hdr).read()
    for d in ('#include "zkv_groth16_set.h"', '#define ZKV_G16_FORM_SNARKJS 0', '#define ZKV_G16_FORM_GNARK 1', '#define ZKV_STATUS_NO_CONTRACT 9',
              '#define ZKV_STATUS_INPUT_NOT_IN_FIELD 10', 'PARITY UNPINNED'):
        assert d in text, d
    from stylus_zkvm_verifiers_amd import _lib, groth16_set, groth16_set_wire as w
    assert set(w.SYMBOLS) == set(NEW)
    assert not set(NEW) & set(_lib.SYMBOLS) and not set(NEW) & set(groth16_set.SYMBOLS)
    for name in NEW:
        assert hasattr(L, name), name
    assert (w.FORM_SNARKJS, w.FORM_GNARK, w.STATUS_NO_CONTRACT, w.STATUS_INPUT_NOT_IN_FIELD) == (gm.FORM_SNARKJS, gm.FORM_GNARK, gm.NO_CONTRACT, gm.NOT_IN_FIELD)
    import stylus_zkvm_verifiers_amd as zkv
    assert zkv.Groth16DeployedSet is w.Groth16DeployedSet


def test_new_status_values_collide_with_no_other_header():
    """Every ZKV_STATUS_* of every header under include/: a value has one name, but for ROUTE_NOT_FOUND, which two routers share."""
    seen = {}
    for f in sorted(os.listdir(os.path.join(ROOT, 'include'))):
        for name, val in re.findall(r'#define\s+(ZKV_STATUS_[A-Z_0-9]+)\s+(\d+)', open(os.path.join(ROOT, 'include', f)).read()):
            seen.setdefault(int(val), set()).add(name)
    assert seen[9] == {'ZKV_STATUS_NO_CONTRACT'} and seen[10] == {'ZKV_STATUS_INPUT_NOT_IN_FIELD'}
    assert all(len(v) == 1 for v in seen.values()) and sorted(seen) == list(range(11))


def test_selector_strings_where_the_decimal_width_of_n_changes(L):
    from stylus_zkvm_verifiers_amd import _lib, groth16_set_wire as w
    raw = _lib.lib()
    for form in (gm.FORM_SNARKJS, gm.FORM_GNARK):
        for n in (1, 9, 10, 99, 100, 128):
            o = C.create_string_buffer(4)
            assert L.zkv_groth16_set_call_selector(form, n, o) == 0
            assert o.raw == gm.selector(form, n) == w.selector(form, n) == w.Groth16DeployedSet.selector(form, n), (form, n)
            p = C.create_string_buffer(4)
            assert raw.zkv_abi_function_selector(gm.signature(form, n).encode(), p) == 0 and p.raw == o.raw      # the library's own keccak
        for n in (0, 129, 1 << 40):
            assert L.zkv_groth16_set_call_selector(form, n, C.create_string_buffer(4)) == INVALID_ARG
        assert L.zkv_groth16_set_call_selector(form, 1, None) == INVALID_ARG
    assert L.zkv_groth16_set_call_selector(2, 1, C.create_string_buffer(4)) == INVALID_ARG
    assert gm.selector(gm.FORM_SNARKJS, 1).hex() == '43753b4d'       # snarkjs' one-signal verifier, as deployed contracts show it
    assert len({gm.selector(f, n) for f in (0, 1) for n in range(1, 129)}) == 256
    proof, sig = bytes(range(256)), [bytes([7]) * 32, bytes([9]) * 32]
    assert w.encode_call(gm.FORM_GNARK, proof, sig) == gm.encode(gm.FORM_GNARK, proof, sig) == gm.selector(gm.FORM_GNARK, 2) + proof + sig[0] + sig[1]
    with pytest.raises(ValueError):
        w.encode_call(gm.FORM_GNARK, proof[:-1], sig)
    with pytest.raises(ValueError):
        w.selector(gm.FORM_GNARK, 0)


def test_creation_refuses_duplicate_addresses_and_unknown_forms(L):
    import stylus_zkvm_verifiers_amd as zkv
    from stylus_zkvm_verifiers_amd import _lib
    a, b = bytes(range(20)), bytes(range(1, 21))
    good = [(_vk(3), 3, 0, a, 0), (_vk(3), 3, 1, b, 1), (_vk(1), 1, 1, bytes(20), 0)]
    h = _create(L, good)
    assert h and _lib.lib().zkv_ctx_vm(h) == 7 and L.zkv_groth16_set_size(h) == 3 and L.zkv_groth16_set_signal_stride(h) == 64
    _lib.lib().zkv_ctx_destroy(h)
    assert not _create(L, [good[0], (_vk(2), 2, 1, a, 1)])                        # two keys, one address
    assert not _create(L, [good[0], good[1], (_vk(2), 2, 1, b, 0)])               # ... not next to each other before the sort
    for form in (2, 255):
        assert not _create(L, [good[0], (_vk(2), 2, 1, b, form)])
    assert not _create(L, [(_vk(2), 2, 2, a, 0)])                                 # what zkv_groth16_set_create refuses
    assert not _create(L, [(_vk(1), 0, 1, a, 0)])
    k = (C.c_char_p * 1)(_vk(2)); n = (C.c_size_t * 1)(2); vm = (C.c_int * 1)(1)
    assert not L.zkv_groth16_set_create_deployed(1, k, n, vm, None, bytes(1), 0)
    assert not L.zkv_groth16_set_create_deployed(1, k, n, vm, a, None, 0)
    assert not L.zkv_groth16_set_create_deployed(0, k, n, vm, a, bytes(1), 0)
    with pytest.raises(ValueError):
        zkv.Groth16DeployedSet([good[0], (_vk(2), 2, 1, a, 1)])
    with pytest.raises(ValueError):
        zkv.Groth16DeployedSet([(_vk(2), 2, 1, a, 2)])
    with pytest.raises(ValueError):
        zkv.Groth16DeployedSet([(_vk(2), 2, 1, a[:19], 0)])
    # the same key twice under two addresses is a set like any other
    s = zkv.Groth16DeployedSet([good[0], (_vk(3), 3, 0, b, 1)])
    assert s.size() == 2 and s.last_call_counts() == [0, 0, 0, 0]
    s.close()


def test_wrong_contexts_bad_arguments_empty_batches_and_returndata(L):
    import stylus_zkvm_verifiers_amd as zkv
    from stylus_zkvm_verifiers_amd import _lib
    raw = _lib.lib()
    a, b = bytes(range(20)), bytes(range(1, 21))
    plain = zkv.Groth16VerifierSet([(_vk(2), 2, 1)])
    g16 = raw.zkv_groth16_ctx_create(_vk(2), 2, 1, 0)
    out = C.create_string_buffer(96); ln = C.c_uint32(7); rev = C.c_uint8(7); cnt = (C.c_uint64 * 4)()
    for h in (None, plain._h, g16):                                  # a set made by the old constructor answers WRONG_CTX
        assert L.zkv_groth16_set_eth_call_batch(h, 0, None, None, None, None, None, None, None) == WRONG_CTX
        assert L.zkv_groth16_set_eth_call_batch_dev(h, 0, None, None, None, 0, None, None, None) == WRONG_CTX
        assert L.zkv_groth16_set_eth_call_returndata(h, 0, 0, out, C.byref(ln), C.byref(rev)) == WRONG_CTX
        assert L.zkv_groth16_set_last_call_counts(h, cnt) == WRONG_CTX
    raw.zkv_ctx_destroy(g16); plain.close()
    s = zkv.Groth16DeployedSet([(_vk(3), 3, 0, a, gm.FORM_SNARKJS), (_vk(2), 2, 1, b, gm.FORM_GNARK)])
    h = s._h
    assert L.zkv_groth16_set_eth_call_batch(h, 0, None, None, None, None, None, None, None) == 0       # empty batches need no device
    assert L.zkv_groth16_set_eth_call_batch_dev(h, 0, None, None, None, 0, None, None, None) == 0
    assert s.eth_call_batch([], [])[1] == []
    off = np.array([0, 8], dtype=np.uint64); r1 = np.zeros(1, np.uint8); d1 = np.zeros(96, np.uint8); l1 = np.zeros(1, np.uint32)
    P = lambda x: x.ctypes.data
    args = [a, bytes(64), P(off), P(r1), P(d1), P(l1)]
    for drop in range(6):
        assert L.zkv_groth16_set_eth_call_batch(h, 1, *[None if j == drop else v for j, v in enumerate(args)], None) == INVALID_ARG, drop
    assert L.zkv_groth16_set_eth_call_batch(h, 0xFFFFFFF1, *args, None) == INVALID_ARG
    for drop in (0, 1, 2, 4):
        dargs = [8, 8, 8, 64, 8, None, None]
        dargs[drop] = None
        assert L.zkv_groth16_set_eth_call_batch_dev(h, 1, *dargs) == INVALID_ARG, drop
    assert L.zkv_groth16_set_eth_call_batch_dev(h, 0xFFFFFFF1, 8, 8, 8, 64, 8, None, None) == INVALID_ARG
    assert L.zkv_groth16_set_last_call_counts(h, None) == INVALID_ARG
    f = C.c_float(0)
    assert raw.zkv_ctx_last_wire_ms(h, C.byref(f)) == -2             # no eth_call batch has run (no device was touched)
    # return data of every status, by the key's form
    model = gm.Contracts([(_vk(3), 3, 0, a, gm.FORM_SNARKJS), (_vk(2), 2, 1, b, gm.FORM_GNARK)])
    for st in range(256):
        for key in (0, 1, 2, gm.NO_KEY):
            out = C.create_string_buffer(b'\xee' * 97); ln = C.c_uint32(77); rev = C.c_uint8(77)
            rc = L.zkv_groth16_set_eth_call_returndata(h, key, st, out, C.byref(ln), C.byref(rev))
            assert out.raw[96:97] == b'\xee'
            if st in (gm.NO_CONTRACT, gm.BAD_CALLDATA) or (st in (gm.OK, gm.FAILED, gm.NOT_IN_FIELD) and key < 2):
                assert rc == 0 and (bool(rev.value), out.raw[:ln.value]) == model.returndata(key, st) == s.eth_call_returndata(key, st), (st, key)
            else:
                assert rc == INVALID_ARG, (st, key)
    assert model.returndata(1, gm.FAILED) == (True, gm.PROOF_INVALID) and model.returndata(1, gm.NOT_IN_FIELD) == (True, gm.NOT_IN_FIELD_ERROR)
    assert model.returndata(0, gm.NOT_IN_FIELD) == (False, bytes(32)) and model.returndata(1, gm.OK) == (False, b'')
    for bad in (None,):
        assert L.zkv_groth16_set_eth_call_returndata(h, 0, 0, bad, C.byref(ln), C.byref(rev)) == INVALID_ARG
    assert L.zkv_groth16_set_eth_call_returndata(h, 0, 0, out, None, C.byref(rev)) == INVALID_ARG
    assert L.zkv_groth16_set_eth_call_returndata(h, 0, 0, out, C.byref(ln), None) == INVALID_ARG
    s.close()


def test_case_list_covers_every_class_by_the_oracle_alone(world):
    """What the GPU fixture asserts, here on the CPU: the seeded list accepts and rejects in every class, under both forms."""
    keys, reqs, model, want = world
    gm.check_coverage(keys, reqs, want)
    assert sorted({k[1] for k in keys}) == [1, 2, 3, 7, 17, 129]
    for n in (1, 3, 63, 64, 65, 3000):
        to, blob, off, exp = gm.batch(reqs, want, n, 100 + n)
        assert len(to) == 20 * n and len(off) == n + 1 and len(exp) == n and int(off[-1]) == len(blob)
        assert sum(gm.counts(exp)) == n
        if n >= 3:
            o = off.astype(np.int64)
            assert (o[1:] < o[:-1]).sum() == 1 and (o > len(blob)).sum() == 1      # one request backwards, one past the blob


def _decode(hs, model, to, blob, off, shift, stride, form):
    n = len(off) - 1
    tab = model.table()
    key = np.full(n, 0xEEEEEEEE, np.uint32); rkey = np.full(n, 0xEEEEEEEE, np.uint32)
    proofs = np.full((n, 256), 0xEE, np.uint8); rows = np.full((n, stride), 0xEE, np.uint8)
    verdict = np.full(n, 0xEE, np.uint8); big = np.full(n, 0xEE, np.uint8)
    assert hs.hsgsw_decode(n, to + b'\0', blob + b'\0', len(blob), off.ctypes.data, shift, tab.ctypes.data, len(tab), stride, key.ctypes.data, rkey.ctypes.data,
                           proofs.ctypes.data, rows.ctypes.data, verdict.ctypes.data, big.ctypes.data, form) == 0
    return key, rkey, proofs, rows, verdict, big


def test_kernel_decode_function_equals_the_model(hs, world):
    """The functions k_gset_wire_decode is made of -- in the plain form, a request start to end, and in the kernel's wavefront form, 64
    lanes resolving their requests and then copying the calls together -- on the whole case list and on shuffled batches with the two
    offset cases, the blob at every alignment: verdicts, resolved and placement keys, the copied bytes and the in-field bytes; nothing is
    written for a request that is not a canonical call, and nothing past a key's own signals."""
    keys, reqs, model, want = world
    stride = 32 * (max(k[1] for k in keys) - 1)
    batches = [(b''.join(r[2] for r in reqs), b''.join(r[3] for r in reqs), np.cumsum([0] + [len(r[3]) for r in reqs]).astype(np.uint64), want)]
    batches += [gm.batch(reqs, want, n, 300 + n) for n in (1, 63, 64, 65, 700)]
    seen = set()
    for to, blob, off, exp in batches:
        for shift, form in ((0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (1, 1), (2, 1), (3, 1)):
            key, rkey, proofs, rows, verdict, big = _decode(hs, model, to, blob, off, shift, stride, form)
            for i, (st, rk, _, _) in enumerate(exp):
                o0, o1 = int(off[i]), int(off[i + 1])
                inside = o0 <= o1 <= len(blob)
                v, j, proof, sig, ge = model.decode(to[20 * i:20 * i + 20], blob[o0:o1]) if inside else (gm.BAD_CALLDATA, gm.NO_KEY, None, None, False)
                assert (verdict[i], rkey[i], big[i]) == (v, j, int(ge)) and rkey[i] == rk, (i, shift)
                assert key[i] == (j if v == 0 and not ge else gm.NO_KEY), (i, shift)
                assert (v if v else gm.NOT_IN_FIELD if ge else st) == st
                if v == 0:
                    assert proofs[i].tobytes() == proof and rows[i, :32 * len(sig)].tobytes() == b''.join(sig), (i, shift)
                    assert (rows[i, 32 * len(sig):] == 0xEE).all()
                else:
                    assert (proofs[i] == 0xEE).all() and (rows[i] == 0xEE).all(), (i, shift)
                seen.add((int(v), bool(ge), inside))
    assert seen == {(0, False, True), (0, True, True), (gm.BAD_CALLDATA, False, True), (gm.NO_CONTRACT, False, True), (gm.BAD_CALLDATA, False, False)}
