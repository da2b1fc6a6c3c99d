"""eth_call batches on a PLONK key set of deployed contracts (include/zkv_plonk_set_wire.h) without a device: the
header against the library's exports, the selector and the five Error(string) byte strings against the model's
(tests/plonk_set_wire_model.py), creation's refusals, the case list against the fixture's recorded verdicts, and the rule header the
kernels run (csrc/zkv_wire_pset.h, compiled for the host, also as a stand-alone program under the address and undefined-behaviour
sanitizers) against the model on that list.  PARITY UNPINNED: the reference holds no PLONK code and no contract shell."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import plonk_set_wire_model as pm
import plonk_trapdoor_keys as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ['zkv_plonk_set_create_deployed', 'zkv_plonk_set_call_selector', 'zkv_plonk_set_eth_call_batch', 'zkv_plonk_set_eth_call_batch_dev',
       'zkv_plonk_set_eth_call_returndata', 'zkv_plonk_set_last_call_counts']
WRONG_CTX, INVALID_ARG = -5, -1
CSRC = os.path.join(ROOT, 'stylus_zkvm_verifiers_amd', 'csrc')
SIM = os.path.join(HERE, 'host_sim', 'host_sim_pset_wire.cpp')


@pytest.fixture(scope='module')
def L():
    from stylus_zkvm_verifiers_amd import plonk_set_wire
    return plonk_set_wire.lib()


@pytest.fixture(scope='module')
def world():
    fx = pm.fixture()
    keys = pm.deployed_set(fx)
    reqs = pm.requests(keys, fx)
    model = pm.Contracts(keys)
    return fx, keys, reqs, model, pm.expected(model, reqs)


def _sim_deps():
    return [SIM] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.h')]


@pytest.fixture(scope='module')
def hs():
    lib = os.path.join(HERE, 'host_sim', 'libhost_sim_pset_wire.so')
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in _sim_deps()):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-Wno-unknown-pragmas', '-o', lib, SIM])
    S = C.CDLL(lib)
    S.hspsw_decode.argtypes = [C.c_uint64, C.c_char_p, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p] * 8 + [C.c_int]
    return S


def _names(path):
    return set(re.findall(r'\b(zkv_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)))


def _vk(nb=2, nc=0):
    return T.vk_bytes(T.shape_key(nb, nc))


def _create(L, keys):
    k = len(keys)
    return L.zkv_plonk_set_create_deployed(k, (C.c_char_p * k)(*[vk for vk, _ in keys]), (C.c_size_t * k)(*[len(vk) for vk, _ in keys]),
                                           b''.join(a for _, a in keys), 0)


def test_header_declares_the_new_symbols_and_the_library_exports_them(L):
    hdr = os.path.join(ROOT, 'include', 'zkv_plonk_set_wire.h')
    assert _names(hdr) == set(NEW)
    text = open(hdr).read()
    for d in ('#include "zkv_plonk_set.h"', '#include "zkv_groth16_set_wire.h"', '#define ZKV_PLONK_REVERT_NONE 0', '#define ZKV_PLONK_REVERT_INPUT_COUNT 1',
              '#define ZKV_PLONK_REVERT_INPUT_RANGE 2', '#define ZKV_PLONK_REVERT_PROOF_SIZE 3', '#define ZKV_PLONK_REVERT_OPENING_RANGE 4',
              '#define ZKV_PLONK_REVERT_EC_OPERATION 5', '#define ZKV_PLONK_RETURNDATA_STRIDE 128', 'PARITY UNPINNED'):
        assert d in text, d
    assert not re.findall(r'#define\s+ZKV_STATUS_', text)                     # the revert causes travel in the reason byte: no new status number
    assert '#define ZKV_RETURNDATA_STRIDE 96' in open(os.path.join(ROOT, 'include', 'zkv.h')).read()
    from stylus_zkvm_verifiers_amd import _lib, plonk_set, plonk_set_wire as w
    assert set(w.SYMBOLS) == set(NEW)
    assert not set(NEW) & set(_lib.SYMBOLS) and not set(NEW) & set(plonk_set.SYMBOLS)
    for name in NEW:
        assert hasattr(L, name), name
    assert (w.STATUS_NO_CONTRACT, w.STATUS_INPUT_NOT_IN_FIELD, w.STATUS_INVALID_PROOF_DATA, w.STATUS_BAD_CALLDATA, w.RETURNDATA_STRIDE) == \
        (pm.NO_CONTRACT, pm.NOT_IN_FIELD, pm.INVALID_PROOF_DATA, pm.BAD_CALLDATA, pm.STRIDE)
    assert (w.REVERT_NONE, w.REVERT_INPUT_COUNT, w.REVERT_INPUT_RANGE, w.REVERT_PROOF_SIZE, w.REVERT_OPENING_RANGE, w.REVERT_EC_OPERATION) == tuple(range(6))
    import stylus_zkvm_verifiers_amd as zkv
    assert zkv.PlonkDeployedSet is w.PlonkDeployedSet and 'PlonkDeployedSet' in zkv.__all__


def test_status_numbers_of_all_headers_are_still_0_to_10():
    """What tests/test_groth16_set_wire_host.py demands of every header under include/, restated here for the new one."""
    seen = {}
    for f in sorted(os.listdir(os.path.join(ROOT, 'include'))):
        for name, val in re.findall(r'#define\s+(ZKV_STATUS_[A-Z_0-9]+)\s+(\d+)', open(os.path.join(ROOT, 'include', f)).read()):
            seen.setdefault(int(val), set()).add(name)
    assert sorted(seen) == list(range(11)) and all(len(v) == 1 for v in seen.values())


def test_selector_is_the_keccak_of_the_signature(L):
    from stylus_zkvm_verifiers_amd import _lib, plonk_set_wire as w
    o = C.create_string_buffer(4)
    assert L.zkv_plonk_set_call_selector(o) == 0
    assert o.raw == pm.selector() == w.selector() == w.PlonkDeployedSet.selector() == bytes.fromhex('7e4f7a8a')
    p = C.create_string_buffer(4)
    assert _lib.lib().zkv_abi_function_selector(pm.SIGNATURE.encode(), p) == 0 and p.raw == o.raw          # the library's own keccak
    assert pm.error_selector() == bytes.fromhex('08c379a0')
    assert L.zkv_plonk_set_call_selector(None) == INVALID_ARG
    proof, pub = bytes(range(256)) * 3, [bytes([7]) * 32, bytes([9]) * 32]
    assert w.encode_call(proof, pub) == pm.encode(proof, pub) and len(w.encode_call(proof, pub)) == 4 + 96 + 768 + 32 + 64
    assert w.encode_call(proof[:5], [3]) == pm.encode(proof[:5], [pm.word(3)]) and pm.parse(pm.encode(proof[:5], [pm.word(3)])) == (proof[:5], [pm.word(3)])
    with pytest.raises(ValueError):
        w.encode_call(proof, [bytes(31)])


def test_the_five_error_strings_and_every_status_reason_pair(L):
    from stylus_zkvm_verifiers_amd import plonk_set_wire as w
    texts = {1: b'wrong number of public inputs', 2: b'inputs are bigger than r', 3: b'wrong proof size', 4: b'openings bigger than r', 5: b'error ec operation'}
    assert [len(texts[r]) for r in range(1, 6)] == [29, 24, 16, 22, 18]
    for r, msg in texts.items():
        st = pm.NOT_IN_FIELD if r == 2 else pm.INVALID_PROOF_DATA
        rev, data = w.returndata(st, r)
        exact = bytes.fromhex('08c379a0') + (0x20).to_bytes(32, 'big') + len(msg).to_bytes(32, 'big') + msg + bytes(32 - len(msg))
        assert rev and data == exact == pm.error_data(r) and len(data) == 100, r
    ok = {(pm.OK, 0), (pm.FAILED, 0), (pm.BAD_CALLDATA, 0), (pm.NO_CONTRACT, 0), (pm.NOT_IN_FIELD, 2)} | {(pm.INVALID_PROOF_DATA, r) for r in (1, 3, 4, 5)}
    for st in range(256):
        for rs in list(range(8)) + [255]:
            out = C.create_string_buffer(b'\xee' * 129); ln = C.c_uint32(77); rev = C.c_uint8(77)
            rc = L.zkv_plonk_set_eth_call_returndata(st, rs, out, C.byref(ln), C.byref(rev))
            assert out.raw[128:129] == b'\xee'
            if (st, rs) in ok:
                assert rc == 0 and (bool(rev.value), out.raw[:ln.value]) == pm.returndata(st, rs) == w.PlonkDeployedSet.eth_call_returndata(st, rs), (st, rs)
            else:
                assert rc == INVALID_ARG, (st, rs)
    assert pm.returndata(pm.OK, 0) == (False, (1).to_bytes(32, 'big')) and pm.returndata(pm.FAILED, 0) == (False, bytes(32))
    assert pm.returndata(pm.NO_CONTRACT, 0) == (False, b'') and pm.returndata(pm.BAD_CALLDATA, 0) == (True, b'')
    out = C.create_string_buffer(128); ln = C.c_uint32(0); rev = C.c_uint8(0)
    assert L.zkv_plonk_set_eth_call_returndata(0, 0, None, C.byref(ln), C.byref(rev)) == INVALID_ARG
    assert L.zkv_plonk_set_eth_call_returndata(0, 0, out, None, C.byref(rev)) == INVALID_ARG
    assert L.zkv_plonk_set_eth_call_returndata(0, 0, out, C.byref(ln), None) == INVALID_ARG
    with pytest.raises(ValueError):
        w.returndata(pm.INVALID_PROOF_DATA, 2)


def test_creation_refuses_duplicate_addresses_and_what_the_plain_set_refuses(L):
    import stylus_zkvm_verifiers_amd as zkv
    from stylus_zkvm_verifiers_amd import _lib
    a, b, c = bytes(range(20)), bytes(range(1, 21)), bytes(20)
    good = [(_vk(2, 0), a), (_vk(2, 1), b), (_vk(0, 0), c)]
    h = _create(L, good)
    assert h and _lib.lib().zkv_ctx_vm(h) == 10 and L.zkv_plonk_set_size(h) == 3
    assert L.zkv_plonk_set_proof_stride(h) == 864 and L.zkv_plonk_set_input_stride(h) == 64
    _lib.lib().zkv_ctx_destroy(h)
    assert not _create(L, [good[0], (_vk(3, 0), a)])                              # two keys, one address
    assert not _create(L, [good[0], good[1], (_vk(3, 0), a)])                     # ... not next to each other before the sort
    assert not _create(L, [(_vk(2, 0)[:-1], a)])                                  # what zkv_plonk_set_create refuses
    k = (C.c_char_p * 1)(_vk()); n = (C.c_size_t * 1)(len(_vk()))
    assert not L.zkv_plonk_set_create_deployed(1, k, n, None, 0)
    assert not L.zkv_plonk_set_create_deployed(1, None, n, a, 0)
    assert not L.zkv_plonk_set_create_deployed(1, k, None, a, 0)
    assert not L.zkv_plonk_set_create_deployed(0, k, n, a, 0)
    with pytest.raises(ValueError):
        zkv.PlonkDeployedSet([good[0], (_vk(3, 0), a)])
    with pytest.raises(ValueError):
        zkv.PlonkDeployedSet([(_vk(), a[:19])])
    with pytest.raises(ValueError):
        zkv.PlonkDeployedSet([])
    s = zkv.PlonkDeployedSet([good[0], (_vk(2, 0), b)])                            # one key at two addresses is a set like any other
    assert s.size() == 2 and s.last_call_counts() == [0] * 8 and s.shapes == [(2, 0, 768)] * 2
    s.close()


def test_wrong_contexts_bad_arguments_and_empty_batches(L):
    import stylus_zkvm_verifiers_amd as zkv
    from stylus_zkvm_verifiers_amd import _lib
    raw = _lib.lib()
    a = bytes(range(20))
    plain = zkv.PlonkVerifierSet([_vk()])
    gset = zkv.Groth16DeployedSet([(bytes(448 + 128), 2, 1, a, 0)])
    cnt = (C.c_uint64 * 8)()
    for h in (None, plain._h, gset._h):                               # a set made by zkv_plonk_set_create answers WRONG_CTX
        assert L.zkv_plonk_set_eth_call_batch(h, 0, None, None, None, None, None, None, None, None) == WRONG_CTX
        assert L.zkv_plonk_set_eth_call_batch_dev(h, 0, None, None, None, 0, None, None, None, None) == WRONG_CTX
        assert L.zkv_plonk_set_last_call_counts(h, cnt) == WRONG_CTX
    plain.close(); gset.close()
    s = zkv.PlonkDeployedSet([(_vk(), a)])
    h = s._h
    assert L.zkv_plonk_set_eth_call_batch(h, 0, None, None, None, None, None, None, None, None) == 0       # empty batches need no device
    assert L.zkv_plonk_set_eth_call_batch_dev(h, 0, None, None, None, 0, None, None, None, None) == 0
    assert s.eth_call_batch([], [])[1] == []
    off = np.array([0, 8], dtype=np.uint64); r1 = np.zeros(1, np.uint8); d1 = np.zeros(128, np.uint8); l1 = np.zeros(1, np.uint32)
    P = lambda x: x.ctypes.data
    args = [a, bytes(64), P(off), P(r1), P(d1), P(l1)]
    for drop in range(6):
        assert L.zkv_plonk_set_eth_call_batch(h, 1, *[None if j == drop else v for j, v in enumerate(args)], None, None) == INVALID_ARG, drop
    assert L.zkv_plonk_set_eth_call_batch(h, 0xFFFFFFF1, *args, None, None) == INVALID_ARG
    for drop in (0, 1, 2, 4):
        dargs = [8, 8, 8, 64, 8, None, None, None]
        dargs[drop] = None
        assert L.zkv_plonk_set_eth_call_batch_dev(h, 1, *dargs) == INVALID_ARG, drop
    assert L.zkv_plonk_set_eth_call_batch_dev(h, 0xFFFFFFF1, 8, 8, 8, 64, 8, None, None, None) == INVALID_ARG
    assert L.zkv_plonk_set_last_call_counts(h, None) == INVALID_ARG
    f = C.c_float(0)
    assert raw.zkv_ctx_last_wire_ms(h, C.byref(f)) == -2             # no eth_call batch has run (no device was touched)
    s.close()


def test_the_rules_split_the_fixture_as_recorded_and_the_list_covers_every_class(world):
    """By the rules alone the 1,019 fixture cases split into 18 placed-OK, 771 placed-failed, 32 inputs >= r, 117 openings >= r and 81 EC,
    and every case the rules leave unplaced has verdict 0 on record: the classification never contradicts the core."""
    fx, keys, reqs, model, want = world
    split = {}
    for sh in fx['shapes']:
        for name, vk, proof, pub, verdict, _ in T.fixture_cases(sh):
            reason = pm.sanity(sh['nb_public'], sh['n_c'], proof, pub)
            assert reason == 0 or verdict == 0, (sh['nb_public'], sh['n_c'], name)
            split[(reason, verdict)] = split.get((reason, verdict), 0) + 1
    assert split == {(0, 1): 18, (0, 0): 771, (2, 0): 32, (4, 0): 117, (5, 0): 81}
    pm.check_coverage(model, reqs, want)
    assert len(keys) == 24 and sorted(set(model.shapes)) == sorted(T.SHAPES)
    for n in (1, 3, 63, 64, 65, 3000):
        to, blob, off, exp = pm.batch(reqs, want, n, 100 + n, shift=n % 4)
        assert len(to) == 20 * n and len(off) == n + 1 and len(exp) == n and int(off[-1]) == len(blob) and int(off[0]) == n % 4
        assert sum(pm.counts(exp)[:3]) + sum(pm.counts(exp)[3:]) == n
        if n >= 3:
            o = off.astype(np.int64)
            assert (o[1:] < o[:-1]).sum() == 1 and (o > len(blob)).sum() == 1      # one request backwards, one past the blob


def _decode(hs, model, to, blob, off, shift, ps, ins, form):
    n = len(off) - 1
    tab = model.table()
    key = np.full(n, 0xEEEEEEEE, np.uint32); rkey = np.full(n, 0xEEEEEEEE, np.uint32)
    proofs = np.full((n, ps), 0xEE, np.uint8); rows = np.full((n, ins), 0xEE, np.uint8)
    verdict, reason, npt, ec = (np.full(n, 0xEE, np.uint8) for _ in range(4))
    assert hs.hspsw_decode(n, to + b'\0', blob + b'\0', len(blob), off.ctypes.data, shift, tab.ctypes.data, len(tab), int.from_bytes(pm.selector(), 'big'), ps, ins,
                           key.ctypes.data, rkey.ctypes.data, proofs.ctypes.data, rows.ctypes.data, verdict.ctypes.data, reason.ctypes.data, npt.ctypes.data,
                           ec.ctypes.data, form) == 0
    return key, rkey, proofs, rows, verdict, reason, npt, ec


def test_kernel_rule_header_equals_the_model(hs, world):
    """The functions k_pset_wire_decode and k_pset_wire_points are made of -- in the plain form, a request start to end, and in the
    kernel's wavefront form, 64 lanes resolving their requests and then copying the calls together -- on the whole case list and on
    shuffled batches with the two offset cases, the blob at every alignment: verdicts, resolved and placement keys, reasons, the copied
    bytes with zeros behind a short proof; nothing is written for a request that did not pass the length rules, and nothing past a key's
    own inputs."""
    fx, keys, reqs, model, want = world
    ps, ins = 864, 32 * 128
    batches = [(b''.join(r[2] for r in reqs), b''.join(r[3] for r in reqs), np.cumsum([0] + [len(r[3]) for r in reqs]).astype(np.uint64), want)]
    batches += [pm.batch(reqs, want, n, 300 + n) for n in (1, 63, 64, 65, 700)]
    seen = set()
    for to, blob, off, exp in batches:
        for shift in range(4):
            for form in (0, 1):
                key, rkey, proofs, rows, verdict, reason, npt, ec = _decode(hs, model, to, blob, off, shift, ps, ins, form)
                for i, (st, rs, rk, _, _) in enumerate(exp):
                    o0, o1 = int(off[i]), int(off[i + 1])
                    inside = o0 <= o1 <= len(blob)
                    v, j, r, proof, pub = model.classify(to[20 * i:20 * i + 20], blob[o0:o1]) if inside else (pm.BAD_CALLDATA, pm.NO_KEY, 0, None, None)
                    got_r = int(reason[i]) or (pm.R_EC if ec[i] else 0)
                    assert (verdict[i], rkey[i], got_r) == (v, j, r) and (rkey[i], got_r) == (rk, rs), (i, shift, form)
                    assert key[i] == (j if v == 0 and r == 0 else pm.NO_KEY), (i, shift, form)
                    assert npt[i] == (9 + model.shapes[j][1] if v == 0 and r in (0, pm.R_EC) else 0)
                    lengths = v == 0 and len(pub) == model.shapes[j][0] and len(proof) == 32 * (24 + 3 * model.shapes[j][1])
                    if lengths:
                        assert proofs[i, :len(proof)].tobytes() == proof and not proofs[i, len(proof):].any(), (i, shift, form)
                        assert rows[i, :32 * len(pub)].tobytes() == b''.join(pub) and (rows[i, 32 * len(pub):] == 0xEE).all(), (i, shift, form)
                    else:
                        assert (proofs[i] == 0xEE).all() and (rows[i] == 0xEE).all(), (i, shift, form)
                    seen.add((int(v), int(r), inside))
    assert seen == {(0, r, True) for r in range(6)} | {(pm.BAD_CALLDATA, 0, True), (pm.NO_CONTRACT, 0, True), (pm.BAD_CALLDATA, 0, False)}


def test_stand_alone_simulation_under_the_sanitizers(tmp_path):
    """The same source as a program of its own with -fsanitize=address,undefined, run directly: requests of every kind from an
    exact-size blob at every alignment, in both forms."""
    exe = str(tmp_path / 'hspsw_main')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wno-unknown-pragmas', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-DHSPSW_MAIN', '-o', exe, SIM])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stdout + r.stderr
