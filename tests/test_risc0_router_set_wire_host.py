"""eth_call batches and per-seal methods on a RISC Zero router with a set route, without a GPU (include/zkv_risc0_router_set_wire.h,
DESIGN.md section 17c): the header's symbol set beside its neighbours', wrong contexts and argument errors on both kinds of router before
any device is touched, the fixture against the model alone, and a stand-alone host program (tests/host_sim/host_sim_rzset_wire.cpp, plain
and under the sanitizers, as a child process) that runs the composed decode, the arena placement and the per-claim method choice the
kernels run.  PARITY UNPINNED: the reference holds no router and no set verifier."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import risc0_router_model as rm
import risc0_router_set_model as rsm
import risc0_router_set_wire_model as swm
import risc0_router_wire_model as wm
import set_inclusion_model as sm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'host_sim', 'host_sim_rzset_wire.cpp')
H = bytes.fromhex
NEW = ['zkv_risc0_router_verify_call_ragged_dev', 'zkv_risc0_router_verify_call_ragged', 'zkv_risc0_router_eth_call_ragged_dev',
       'zkv_risc0_router_eth_call_ragged', 'zkv_risc0_router_last_ragged_call_counts']
WRONG_CTX, INVALID_ARG, NO_DEVICE = -5, -1, -2
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
SHAPES = [(f, t) for f in (0, 1) for t in (0, 1)]


@pytest.fixture(scope='module')
def L():
    from stylus_zkvm_verifiers_amd import risc0_router_set_wire
    return risc0_router_set_wire.lib()


@pytest.fixture(scope='module')
def fx():
    return swm.load_fixture(os.path.join(HERE, 'golden', 'risc0_router_set_wire_cases.json'))


@pytest.fixture(scope='module')
def keys(fx):
    return [rm.Key(s) for s in fx['key_seeds']]


def _routes(fx, keys):
    b = fx['builtin']
    return [(H(b['control_root']), H(b['bn254_control_id']))], [k.triple() for k in keys]


@pytest.fixture(scope='module')
def model(fx, keys):
    s = rsm.SetRouter(H(fx['set_id']), *_routes(fx, keys))
    assert [x.hex() for x in s.selectors] == fx['route_selectors'] and s.set_selector.hex() == fx['set_selector']
    for r in fx['submitted_roots']:
        assert s.submit_root(H(r['root']), H(r['seal']))[0] == 0
    return swm.SetWireRouter(s)


def _names(path):
    return set(re.findall(r'\b(zkv_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)))


# ---------------------------------------------------------------- symbol sets
def test_header_declares_exactly_the_five_names_and_the_library_exports_them(L):
    inc = lambda f: os.path.join(ROOT, 'include', f)
    assert _names(inc('zkv_risc0_router_set_wire.h')) == set(NEW)
    text = open(inc('zkv_risc0_router_set_wire.h')).read()
    for d in ('#include "zkv_risc0_router_set.h"', '#include "zkv_risc0_router_wire.h"', 'PARITY UNPINNED', 'OVERLAPPING REQUESTS',
              'calldata_bytes / 32 + 64', '346 bytes per request'):
        assert d in text, d
    assert 'zkv_risc0_router_set_wire.h' in open(inc('zkv_risc0_router_set.h')).read()
    from stylus_zkvm_verifiers_amd import _lib, risc0_router, risc0_router_set, risc0_router_set_wire, risc0_router_wire
    assert set(risc0_router_set_wire.SYMBOLS) == set(NEW)
    for name in NEW:
        assert hasattr(L, name), name
    # the neighbours' symbol sets are what they were
    import test_risc0_router_set_host as pinned                      # the lists that test pins
    neighbours = [('zkv_risc0_router.h', pinned.ROUTER, risc0_router.SYMBOLS), ('zkv_risc0_router_wire.h', pinned.WIRE, risc0_router_wire.SYMBOLS),
                  ('zkv_risc0_router_set.h', pinned.NEW, risc0_router_set.SYMBOLS), ('zkv_risc0_set_inclusion.h', pinned.SETINCL, None)]
    for f, names, table in neighbours:
        assert _names(inc(f)) == set(names) and (table is None or set(table) == set(names)) and not set(names) & set(NEW), f
    main = _names(inc('zkv.h'))
    assert len(main) == 83 and len(_lib.SYMBOLS) == 83 and not main & set(NEW)
    # the header compiles as C beside its neighbours, in either order
    others = ('zkv_risc0_router_set.h', 'zkv_risc0_router_wire.h', 'zkv_sp1_gateway_wire.h')
    for order in ((('zkv_risc0_router_set_wire.h',) + others), (others + ('zkv_risc0_router_set_wire.h',))):
        src = ''.join('#include "%s"\n' % inc(f) for f in order) + 'int main(void) { return ZKV_RISC0_ROUTER_CALL_KIND_BAD - 255 + ZKV_SETINCL_MAX_DEPTH - 64; }\n'
        subprocess.run(['gcc', '-x', 'c', '-fsyntax-only', '-Wall', '-Werror', '-'], input=src.encode(), check=True)


# ---------------------------------------------------------------- contexts and arguments
def test_wrong_contexts_and_argument_errors_on_both_kinds_of_router(L, fx, keys):
    from stylus_zkvm_verifiers_amd import RiscZeroRouter, RiscZeroSetRouter, _lib
    raw = _lib.lib()
    rz = raw.zkv_risc0_ctx_create(bytes(32), bytes(32), 0)
    sp = raw.zkv_sp1_ctx_create(0)
    cnt = (C.c_uint64 * 40)()
    for h in (None, rz, sp):
        assert L.zkv_risc0_router_verify_call_ragged_dev(h, 0, None, None, None, 0, None, None, None, None, None) == WRONG_CTX
        assert L.zkv_risc0_router_verify_call_ragged(h, 0, None, None, None, None, None, None, None) == WRONG_CTX
        assert L.zkv_risc0_router_eth_call_ragged_dev(h, 0, None, None, 0, None, None, None, None) == WRONG_CTX
        assert L.zkv_risc0_router_eth_call_ragged(h, 0, None, None, None, None, None, None) == WRONG_CTX
        assert L.zkv_risc0_router_last_ragged_call_counts(h, cnt) == WRONG_CTX
    plain = RiscZeroRouter(*_routes(fx, keys))
    withset = RiscZeroSetRouter(H(fx['set_id']), *_routes(fx, keys))
    blob = bytes(64)
    ok = np.array([0, 8], dtype=np.uint64); back = np.array([8, 4], dtype=np.uint64)
    r1 = np.zeros(1, np.uint8); d1 = np.zeros(96, np.uint8); l1 = np.zeros(1, np.uint32); s1 = np.zeros(1, np.uint8); v1 = np.zeros(4, np.uint8)
    a32 = np.zeros(32, np.uint8)
    P = lambda a: a.ctypes.data
    f = C.c_float(0)
    for rt, routes in ((plain, 3), (withset, 4)):
        g = rt._h
        # empty batches: nothing to do
        assert L.zkv_risc0_router_verify_call_ragged_dev(g, 0, None, None, None, 0, None, None, None, None, None) == 0
        assert L.zkv_risc0_router_verify_call_ragged(g, 0, None, None, None, None, None, None, None) == 0
        assert L.zkv_risc0_router_eth_call_ragged_dev(g, 0, None, None, 0, None, None, None, None) == 0
        assert L.zkv_risc0_router_eth_call_ragged(g, 0, None, None, None, None, None, None) == 0
        for miss in range(5):                                       # blob, offsets, reverted, return data, lengths: none may be NULL (status may)
            args = [blob, P(ok), P(r1), P(d1), P(l1)]
            args[miss] = None
            assert L.zkv_risc0_router_eth_call_ragged(g, 1, *args, P(s1)) == INVALID_ARG, miss
        assert L.zkv_risc0_router_eth_call_ragged(g, 1, blob, P(back), P(r1), P(d1), P(l1), P(s1)) == INVALID_ARG      # host offsets not monotone
        assert L.zkv_risc0_router_eth_call_ragged(g, 0xFFFFFFF1, blob, P(ok), P(r1), P(d1), P(l1), P(s1)) == INVALID_ARG
        assert L.zkv_risc0_router_eth_call_ragged_dev(g, 1, None, 8, 64, 8, None, None, None) == INVALID_ARG
        assert L.zkv_risc0_router_eth_call_ragged_dev(g, 1, 8, None, 64, 8, None, None, None) == INVALID_ARG
        assert L.zkv_risc0_router_eth_call_ragged_dev(g, 1, 8, 8, 64, None, None, None, None) == INVALID_ARG
        assert L.zkv_risc0_router_eth_call_ragged_dev(g, 0xFFFFFFF1, 8, 8, 64, 8, None, None, None) == INVALID_ARG
        for miss in range(5):                                       # seals, offsets, in_a, in_b, status (the method row and the selectors may be NULL)
            args = [blob, P(ok), P(a32), P(a32), P(s1)]
            args[miss] = None
            assert L.zkv_risc0_router_verify_call_ragged(g, 1, None, *args, P(v1)) == INVALID_ARG, miss
        assert L.zkv_risc0_router_verify_call_ragged(g, 1, None, blob, P(back), P(a32), P(a32), P(s1), P(v1)) == INVALID_ARG
        for miss in range(5):                                       # blob (with bytes in it), offsets, in_a, in_b, status
            args = [8, 8, 8, 8, 8]
            args[miss] = None
            assert L.zkv_risc0_router_verify_call_ragged_dev(g, 1, None, args[0], args[1], 64, args[2], args[3], args[4], None, None) == INVALID_ARG, miss
        assert L.zkv_risc0_router_verify_call_ragged_dev(g, 0xFFFFFFF1, None, 8, 8, 64, 8, 8, 8, None, None) == INVALID_ARG
        assert L.zkv_risc0_router_last_ragged_call_counts(g, None) == INVALID_ARG
        assert L.zkv_risc0_router_last_ragged_call_counts(g, cnt) == 0 and list(cnt[:routes + 3]) == [0] * (routes + 3)
        assert rt.last_call_counts() == [0] * (routes + 3)
        assert rt.eth_call_batch([])[1] == [] and len(rt.verify_call_batch(None, [], [], [])[0]) == 0
        assert raw.zkv_ctx_last_wire_ms(g, C.byref(f)) == NO_DEVICE      # no device was touched by any of this
    # the entry points of zkv_risc0_router_wire.h keep refusing a router with a set route
    assert L.zkv_risc0_router_eth_call_batch(withset._h, 0, None, None, None, None, None, None) == WRONG_CTX
    assert L.zkv_risc0_router_last_call_counts(withset._h, cnt) == WRONG_CTX
    plain.close(); withset.close()
    for h in (rz, sp):
        raw.zkv_ctx_destroy(h)


# ---------------------------------------------------------------- the fixture against the model alone
def test_fixture_holds_the_models_answers_and_covers_the_ground(fx, model):
    cases, items = fx['cases'], fx['items']
    set_sel = H(fx['set_selector'])
    for c in cases:
        rev, data, st, rv, col, kind = model.eth_call(c['calldata'])
        assert (c['reverted'], c['returndata'], c['status'], c['received'], c['column'], c['kind']) == (int(rev), data.hex(), st, rv.hex(), col, kind), c['name']
    is_set = lambda it: H(it['seal'])[:4] == set_sel and len(H(it['seal'])) > 4
    decoded = lambda it: sm.abi_decode_seal(H(it['seal'])[4:])
    for form, method in SHAPES:
        mine = [c for c in cases if (c['form'], c['method']) == (form, method)]
        plain = [items[c['item']] for c in mine if not c['ops']]
        assert {len(H(it['seal'])) for it in plain if not is_set(it)} >= {0, 3, 4, 259, 260, 261, 292}
        shapes = {(len(d[0]), len(d[1])) for d in (decoded(it) for it in plain if is_set(it)) if d is not None}
        assert {d for d, _ in shapes} >= {0, 1, 3, 64, 65}
        for depth in (0, 1, 3, 64, 65):
            assert {n for d, n in shapes if d == depth} >= {0, 4, 259, 260, 261}, depth
        assert any(is_set(it) and decoded(it) is None for it in plain)
        names = ' | '.join(c['name'] for c in mine)
        for need in ('root submitted', 'root not submitted', 'nested', 'unknown selector', 'wrong claim digest' if method else 'another journal digest',
                     'offset 32 more', 'length + 2^32', 'cut to 0 bytes', 'one trailing byte', "the other form's selector", 'path length 2^59',
                     'element 4 of' if form == 0 else 'first padding byte set [set seal', 'element 261 of' if form == 0 else 'last padding byte set [set seal',
                     'is 256 more [keyed route 0, seal of 292 bytes]' if form == 0 else 'padding byte set [keyed route 0, seal of 292 bytes]'):
            assert need in names, (form, method, need)
        sts = {(c['status'], c['column']) for c in mine}
        assert sts >= {(0, swm.SET), (1, swm.SET), (4, swm.SET), (8, swm.SET), (6, swm.BAD), (0, 0), (0, 1), (0, 2)}
        # a malformed set body inside canonical calldata keeps the seal layer's verdict
        assert all(c['status'] == 4 for c in mine if not c['ops'] and 'set seal edited' in c['name'] and 'length 32 less' not in c['name']
                   and decoded(items[c['item']]) is None)
    # a uint8[] element above 255 is bad calldata on either side of byte 260, in a set seal and in a Groth16-route seal
    over = [c for c in cases if ' is 256 more [' in c['name']]
    assert len(over) == 2 * 2 * 6 and all(c['status'] == 6 and c['column'] == swm.BAD for c in over)
    # one claim in all four shapes under one root seal is one root job; a wrong claim digest under it is a straggler
    by = {c['name']: c for c in cases}
    four = [by['%s%s: set seal, shared tree, leaf 0' % (f, t)]['calldata'] for f in 'UB' for t in 'vi']
    got = model.eth_call_batch(four)
    assert [r[2] for r in got['rows']] == [0] * 4 and got['set_counts'] == (4, 1, 1, 0) and got['counts'] == [0, 0, 0, 4, 0, 0, 0]
    strag = [by['%si: set seal, shared tree, leaf 0 with a wrong claim digest (integrity calls only)' % f]['calldata'] for f in 'UB']
    got = model.eth_call_batch(four + strag + [b'\1\2\3'])
    assert [r[2] for r in got['rows']] == [0] * 4 + [1, 1, 6] and got['set_counts'] == (6, 1, 3, 0) and got['counts'] == [0, 0, 0, 6, 0, 0, 1]
    # the decoded-input call: a bad method byte is bad calldata, no set seal, no root job
    d = wm.decode(four[0])
    got = model.verify_call_batch([0, 2, 255, 1], [d[2]] * 4, [d[3]] * 4, [d[4]] * 4)
    assert [r[0] for r in got['rows']] == [0, 6, 6, 1] and got['set_counts'] == (2, 1, 2, 0) and got['counts'] == [0, 0, 0, 2, 0, 0, 2]


# ---------------------------------------------------------------- the host program
def _program(tmp_path, flags, name):
    exe = str(tmp_path / name)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wno-unknown-pragmas'] + flags + ['-o', exe, SRC])
    return exe


def _run(exe, args, lines=None):
    out = subprocess.run([exe] + args, input=''.join(ln + '\n' for ln in lines or []).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stderr.decode()[-2000:])
    assert not out.stderr, out.stderr.decode()[-2000:]
    return out.stdout.decode().splitlines()


def _mutations(set_sel):
    """4,000 seeded mutations, as (shift, calldata): a seal -- a small set seal, a set selector in front of noise, or noise -- with one
    word of its body replaced, in one of the four call shapes with, now and then, one word of the call's own header replaced, an element
    or padding byte set, a byte cut or added."""
    rng = random.Random(0x5E7CA11E)
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))
    values = lambda cur: [0, 1, 31, 32, 33, 0x20, 0x40, 0x60, 0x80, 0xa0, cur, cur + 1, cur - 1, cur + 32, cur - 32, cur + (1 << 32), cur + (1 << 64),
                          cur + (1 << 248), (1 << 32) - 1, 1 << 32, (1 << 59), (1 << 64) - 32, (1 << 256) - 1, rng.randrange(200), rng.randrange(1 << 256)]
    out = []
    for trial in range(4000):
        form, method = rng.randrange(2), rng.randrange(2)
        kind = rng.randrange(8)
        if kind < 5:
            seal = bytearray(set_sel + sm.abi_encode_seal([rb(32) for _ in range(rng.choice([0, 1, 2, 3]))], rb(rng.choice([0, 4, 31, 32, 33, 64, 70]))))
            if rng.randrange(3):
                at = 4 + 32 * rng.randrange((len(seal) - 4) // 32)
                cur = int.from_bytes(seal[at:at + 32], 'big')
                seal[at:at + 32] = (rng.choice(values(cur)) % (1 << 256)).to_bytes(32, 'big')
            if rng.randrange(6) == 0:
                seal = seal[:len(seal) - rng.choice([1, 31, 32])] if rng.randrange(2) else seal + bytes(rng.choice([1, 31, 32]))
        elif kind < 6:
            seal = set_sel + rb(rng.choice([0, 1, 28, 156, 160, 188, 270]))
        else:
            seal = rb(rng.choice([0, 3, 4, 31, 64, 259, 260, 261, 300]))
        cd = bytearray(wm.encode(form, method, bytes(seal), bytes(32), bytes(32) if method == wm.VERIFY else None))
        l_at = 68 if (form, method) == (0, 1) else 100
        edit = rng.randrange(12)
        if edit == 0:
            at = rng.choice([4, 36, l_at])
            cur = int.from_bytes(cd[at:at + 32], 'big')
            cd[at:at + 32] = (rng.choice(values(cur)) % (1 << 256)).to_bytes(32, 'big')
        elif edit == 1 and len(cd) > l_at + 32:
            at = rng.randrange(l_at + 32, len(cd))                       # an element's upper bytes or its value (form U); a seal or padding byte
            cd[at] ^= 1 << rng.randrange(8)
        elif edit == 2:
            del cd[len(cd) - rng.choice([1, 31, 32, 33]):]
        elif edit == 3:
            cd += bytes(rng.choice([1, 31, 32, 33]))
        out.append((trial & 3, bytes(cd)))
    return out


def _want_decode(cd, set_sel):
    d = wm.decode(cd)
    if d is None:
        return '0 0 0 0 0 0 0 0 0 -'
    form, method, seal = d[0], d[1], d[2]
    is_set = len(seal) >= 4 and seal[:4] == set_sel
    kept = len(seal) if form == 1 or is_set else min(len(seal), 260)
    kind = depth = root_len = root_at = 0
    if is_set:
        body = sm.abi_decode_seal(seal[4:])
        kind = 1 if body is None else 2
        if body is not None:
            depth, root_len = len(body[0]), len(body[1])
            root_at = 4 + 128 + 32 * depth + 32
    return '1 %d %d %d %d %d %d %d %d %s' % (form, method, len(seal), kept, kind, depth, root_len, root_at, seal[:min(kept, 260)].hex() or '-')


@pytest.mark.parametrize('flags,name', [([], 'plain'), (SANITIZE, 'san')])
def test_host_program_composed_decode_arena_and_method_choice(tmp_path, fx, flags, name):
    exe = _program(tmp_path, flags, name)
    set_sel = H(fx['set_selector'])
    sels = ' '.join(wm.selector(k >> 1, k & 1).hex() for k in range(4)) + ' ' + set_sel.hex()
    # the composed decode on every golden request at four alignments and on the seeded mutations, from blocks of exactly the request
    reqs = [(shift, c['calldata']) for c in fx['cases'] for shift in (0, 1, 2, 3)] + _mutations(set_sel)
    got = _run(exe, ['decode'], ['%d %s %s' % (shift, sels, cd.hex() or '-') for shift, cd in reqs])
    assert len(got) == len(reqs)
    seen = {}
    for (shift, cd), line in zip(reqs[-4000:], got[-4000:]):
        key = line.split()[0] + line.split()[5]
        seen[key] = seen.get(key, 0) + 1
    assert min(seen.get(k, 0) for k in ('00', '10', '11', '12')) > 150, seen      # bad calldata; no set seal, malformed body, claim
    for (shift, cd), line in zip(reqs, got):
        assert line == _want_decode(cd, set_sel), (shift, len(cd), cd[:140].hex())
    for c in fx['cases']:                                            # the decode's verdict is the fixture's bad-calldata column
        assert (_want_decode(c['calldata'], set_sel)[0] == '0') == (c['status'] == 6 and c['column'] == swm.BAD), c['name']
    # the arena placement: every offset below 4,096 and every decoded length below 600, both head sizes
    assert _run(exe, ['arena', '4096', '600']) == ['ok %d' % (4096 * 2 * 600 * 3)]
    # the per-claim method choice: a method row decides per row, no row means one method for the batch (verify iff it has second inputs)
    rng = random.Random(0x5E7CA11F)
    lines, want = [], []
    for _ in range(200):
        row = bytes(rng.randrange(2) for _ in range(rng.randrange(1, 9)))
        i, have_b = rng.randrange(len(row)), rng.randrange(2)
        use_row = rng.randrange(3) > 0
        lines.append('%s %d %d' % (row.hex() if use_row else '-', 1 if use_row else have_b, i))
        want.append(str(row[i]) if use_row else str(1 - have_b))
    assert _run(exe, ['method'], lines) == want


# ---------------------------------------------------------------- the C++ mirror
def test_cpp_mirror_has_the_set_router(tmp_path):
    src = tmp_path / 'mirror.cpp'
    src.write_text('#include "%s"\n'
                   'int main() { std::vector<zkv::RiscZeroBuiltinRoute> b; std::vector<zkv::RiscZeroKeyedRoute> k; const uint8_t id[32] = {0};\n'
                   '  std::vector<uint8_t> blob, a, bb, st, rv, rev, data, method; std::vector<uint64_t> off; std::vector<uint32_t> len;\n'
                   '  try { zkv::RiscZeroSetRouter r(id, b, k); zkv::RiscZeroRouter& base = r;\n'
                   '    r.verify_call_batch(method, blob, off, a, bb, st, rv); r.eth_call_batch(blob, off, rev, data, len, st);\n'
                   '    r.verify_ragged_dev(0, nullptr, nullptr, 0, nullptr, nullptr, nullptr);\n'
                   '    return (int)r.set_selector().size() + r.submit_root(id, blob) + (int)base.route_count() + (int)r.verify(blob, id, id); }\n'
                   '  catch (const std::exception&) { return 0; } }\n' % os.path.join(ROOT, 'stylus_zkvm_verifiers_amd', 'host', 'zkv_risc0_router.hpp'))
    subprocess.check_call(['g++', '-std=c++17', '-fsyntax-only', '-Wall', '-Werror', str(src)])
