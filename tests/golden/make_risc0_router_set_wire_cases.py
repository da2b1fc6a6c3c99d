#!/usr/bin/env python3
"""Generates tests/golden/risc0_router_set_wire_cases.json: named eth_call requests to a RISC Zero router with a set route -- one built-in
route (the real proof's parameters, real_proofs.json), two keyed trapdoor routes (risc0_router_model.Key) and the set route of a fixed
set-builder image id -- in the four call shapes, with the answers of tests/risc0_router_set_wire_model.py, `submitted_roots` submitted
first.  Every case is an item (seal, image id, journal digest; a verifyIntegrity call carries the claim digest of the two unless the item
names another one), a form, a method and byte edits over the canonical call (tests/wire_util.apply_ops), so that the uint8[] requests
stay small.  PARITY UNPINNED BY CONSTRUCTION: the reference holds no router and no set verifier.

    python tests/golden/make_risc0_router_set_wire_cases.py
"""
import collections
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..', 'oracle'))
sys.path.insert(0, os.path.join(HERE, '..'))
import risc0_router_model as rm              # noqa: E402
import risc0_router_set_model as rsm         # noqa: E402
import risc0_router_set_wire_model as swm    # noqa: E402
import risc0_router_wire_model as wm         # noqa: E402
import set_inclusion_model as sm             # noqa: E402
import spec_model as m                       # noqa: E402

H = bytes.fromhex
KEY_SEEDS = (0x5E73, 0x5E74)
SET_ID = m.sha256(b'risc0 router set wire fixture: set builder image id')
GROTH16_LENGTHS = (0, 3, 4, 259, 260, 261, 292)
DEPTHS = (0, 1, 3, 64, 65)
SHAPES = [(f, t) for f in (wm.FORM_U, wm.FORM_B) for t in (wm.VERIFY, wm.INTEGRITY)]


def rand32(rng):
    return bytes(rng.randrange(256) for _ in range(32))


def patch(seal, at, data):
    return seal[:at] + data + seal[at + len(data):]


def main():
    real = json.load(open(os.path.join(HERE, 'real_proofs.json')))['risc0']
    rng = random.Random(0x5E7CA11D)
    keys = [rm.Key(s) for s in KEY_SEEDS]
    srouter = rsm.SetRouter(SET_ID, [(H(real['control_root']), H(real['bn254_control_id']))], [k.triple() for k in keys])
    model = swm.SetWireRouter(srouter)
    rseal, iid, jd = H(real['seal']), H(real['image_id']), H(real['journal_digest'])
    word = lambda v: int(v).to_bytes(32, 'big')
    wordx = lambda v: word(v).hex()
    root_seal = lambda key, root: key.prove(SET_ID, sm.root_journal(SET_ID, root))
    items, packed, stored = [], [], []          # items as the generator uses them; as the file holds them (an edited seal: base item and edits)

    def item(name, seal, a, b, claim=None):
        it = dict(name=name, seal=bytes(seal).hex(), image_id=bytes(a).hex(), journal_digest=bytes(b).hex())
        if claim is not None:
            it['claim_digest'] = bytes(claim).hex()
        items.append(it)
        packed.append(it)
        return len(items) - 1

    def edited(name, base, ops, inputs=None):
        """The seal of item `base` with byte edits (wire_util.apply_ops), the same inputs unless others are given: the file keeps the edits."""
        a, b = inputs or (H(items[base]['image_id']), H(items[base]['journal_digest']))
        k = item(name, swm.apply_ops(H(items[base]['seal']), ops), a, b)
        packed[k] = dict(name=name, base=base, ops=[list(o) for o in ops])
        if inputs:
            packed[k].update(image_id=a.hex(), journal_digest=b.hex())
        return k

    def claim_with_path(depth):
        a, b = rand32(rng), rand32(rng)
        path = [rand32(rng) for _ in range(depth)]
        return a, b, path, sm.walk(m.receipt_claim_ok_digest(a, b), path)

    # ---- Groth16 routes: every length around the 260 bytes a route reads, both kinds of route; unknown selector
    for n in GROTH16_LENGTHS:
        item('built-in route, seal of %d bytes' % n, (rseal + bytes(32))[:n], iid, jd)
    ka, kb = rand32(rng), rand32(rng)
    kseal = keys[0].prove(ka, kb)
    g_keyed = item('keyed route 0, valid', kseal, ka, kb)
    long_k = item('keyed route 0, seal of 292 bytes', kseal + bytes(32), ka, kb)
    a1, b1 = rand32(rng), rand32(rng)
    item('keyed route 1, valid', keys[1].prove(a1, b1), a1, b1)
    item('unknown selector, real body', b'\xde\xad\xbe\xef' + rseal[4:], iid, jd)
    item('set selector alone', srouter.set_selector, iid, jd)
    # ---- set seals: every depth times every kind of root seal
    for d in DEPTHS:
        a, b, path, root = claim_with_path(d)
        rs = root_seal(keys[d & 1], root)
        full = item('set seal, depth %d, root seal of 260 bytes (keyed route %d)' % (d, d & 1), srouter.encode_seal(path, rs), a, b)
        # the other root seals: the same head and path, the tail from the root seal's length word on replaced
        tail = lambda r: [('truncate', 4 + 128 + 32 * d), ('append', (word(len(r)) + r + bytes(-len(r) % 32)).hex())]
        edited('set seal, depth %d, root seal of 259 bytes' % d, full, tail(rs[:259]))
        edited('set seal, depth %d, root seal of 261 bytes' % d, full, tail(rs + b'\7'))
        edited('set seal, depth %d, root seal of 4 bytes (unknown selector)' % d, full, tail(b'\xca\xfe\xf0\x0d'))
        edited('set seal, depth %d, nested: the root seal is a set seal' % d, full, tail(srouter.encode_seal([], rs)))
        edited('set seal, depth %d, empty root seal, root submitted' % d, full, tail(b''))
        if d <= sm.MAX_DEPTH:
            stored.append((root, root_seal(keys[1], root)))
        edited('set seal, depth %d, empty root seal, root not submitted' % d, full, tail(b''), inputs=(rand32(rng), rand32(rng)))
    # ---- one tree, one root seal: a claim in all four shapes is one root job; a wrong claim digest under it is a straggler
    leaves = [(rand32(rng), rand32(rng)) for _ in range(2)]
    digs = [m.receipt_claim_ok_digest(a, b) for a, b in leaves]
    root, paths = sm.tree_paths([sm.leaf(d) for d in digs])
    assert root == sm.walk(digs[0], paths[0]) == sm.walk(digs[1], paths[1])
    shared = root_seal(keys[0], root)
    g_good = item('set seal, shared tree, leaf 0', srouter.encode_seal(paths[0], shared), *leaves[0])
    item('set seal, shared tree, leaf 1', srouter.encode_seal(paths[1], shared), *leaves[1])
    straggler = item('set seal, shared tree, leaf 0 with a wrong claim digest (integrity calls only)', srouter.encode_seal(paths[0], shared),
                     *leaves[0], claim=rand32(rng))
    item('set seal, shared tree, leaf 0 with another journal digest', srouter.encode_seal(paths[0], shared), leaves[0][0], rand32(rng))
    # ---- every malformed-body class of rzs_parse, over a set seal that verifies (depth 3) and one with a 259-byte root seal
    a, b, path, root = claim_with_path(3)
    good = srouter.encode_seal(path, root_seal(keys[0], root))
    short = srouter.encode_seal(path, root_seal(keys[0], root)[:259])
    long_s = item('set seal, depth 3, valid (base of the edits)', good, a, b)
    short_s = item('set seal, depth 3, root seal of 259 bytes (base of the edits)', short, a, b)
    hx = lambda v: bytes(v).hex()
    for tag, bi in (('valid', long_s), ('259-byte root seal', short_s)):
        base = H(items[bi]['seal'])
        k = 3
        l_at = 4 + 128 + 32 * k
        ln = int.from_bytes(base[l_at:l_at + 32], 'big')
        t = lambda s: 'set seal edited [%s]: %s' % (tag, s)
        for what, ops in (('first word 0x40', [('patch', 4, hx(word(0x40)))]), ('first word + 2^32', [('patch', 4 + 27, '01')]),
                          ('path offset 0x60', [('patch', 36, hx(word(0x60)))]), ('path offset with a high byte', [('patch', 36, '80')]),
                          ('root seal offset 32 more', [('patch', 68, hx(word(0x60 + 32 * k + 32)))]), ('root seal offset + 2^64', [('patch', 68 + 23, '01')]),
                          ('path length one more', [('patch', 100, hx(word(k + 1)))]), ('path length one less', [('patch', 100, hx(word(k - 1)))]),
                          ('path length + 2^32', [('patch', 100 + 27, '01')]), ('path length 2^59 (times 32 wraps)', [('patch', 100, hx(word(1 << 59)))]),
                          ('root seal length one more', [('patch', l_at, hx(word(ln + 1)))]), ('root seal length 32 more', [('patch', l_at, hx(word(ln + 32)))]),
                          ('root seal length 32 less', [('patch', l_at, hx(word(ln - 32)))]), ('root seal length + 2^32', [('patch', l_at + 27, '01')]),
                          ('last byte missing', [('truncate', len(base) - 1)]), ('one trailing byte', [('append', '00')]),
                          ('last word missing', [('truncate', len(base) - 32)]), ('one trailing word', [('append', '00' * 32)])):
            edited(t(what), bi, ops)
        for cut in (5, 36, 163, 164, l_at + 31, l_at + 32):
            edited(t('cut to %d bytes' % cut), bi, [('truncate', cut)])
    edited('set seal malformed [259-byte root seal]: padding byte set', short_s, [('patch', len(short) - 1, '01')])

    for r, s in stored:
        assert srouter.submit_root(r, s)[0] == rsm.OK
    cases = []

    def case(tag, k, form, method, ops=()):
        """tag: what the edits do, or None for the item's canonical call; swm.load_fixture forms the case's name from it."""
        cd = swm.calldata_of(items[k], form, method, ops)
        rev, data, st, rv, col, kind = model.eth_call(cd)
        cases.append(dict(form=form, method=method, item=k, tag=tag, ops=[list(o) for o in ops], calldata_len=len(cd), reverted=int(rev),
                          returndata=data.hex(), status=st, received=rv.hex(), column=col, kind=kind))

    for form, method in SHAPES:
        for k, it in enumerate(items):
            if k != straggler or method == wm.INTEGRITY:
                case(None, k, form, method)
        # every header violation of the calldata layer, over a call with a set seal and one with a Groth16 seal, both verifying
        for k in (g_good, g_keyed):
            it = items[k]
            cd = swm.calldata_of(it, form, method)
            _, _, a_at, at, n = wm.parse_header(cd)
            l_at = at - 32
            tag = lambda t: t
            case(tag('unknown function selector'), k, form, method, [('patch', 0, 'deadbeef')])
            case(tag("the other form's selector"), k, form, method, [('patch', 0, wm.selector(1 - form, method).hex())])
            case(tag("the other method's selector"), k, form, method, [('patch', 0, wm.selector(form, 1 - method).hex())])
            first = int.from_bytes(cd[4:36], 'big')
            case(tag('offset 32 more'), k, form, method, [('patch', 4, wordx(first + 32))])
            case(tag('offset 32 less'), k, form, method, [('patch', 4, wordx(first - 32))])
            case(tag('offset with a high byte'), k, form, method, [('patch', 4, '01')])
            case(tag('offset + 2^64'), k, form, method, [('patch', 4 + 23, '01')])
            if form == wm.FORM_B and method == wm.INTEGRITY:
                case(tag('seal offset in the tuple 0x60'), k, form, method, [('patch', 36, wordx(0x60))])
                case(tag('seal offset in the tuple 0x20'), k, form, method, [('patch', 36, wordx(0x20))])
                case(tag('seal offset in the tuple + 2^32'), k, form, method, [('patch', 36 + 27, '01')])
            case(tag('length + 2^32'), k, form, method, [('patch', l_at + 27, '01')])
            case(tag('length + 2^64'), k, form, method, [('patch', l_at + 23, '01')])
            case(tag('length + 2^255'), k, form, method, [('patch', l_at, '80')])
            step = 1 if form == wm.FORM_U else 32
            case(tag('length more than present'), k, form, method, [('patch', l_at, wordx(n + step))])
            case(tag('length less than present'), k, form, method, [('patch', l_at, wordx(n - step))])
            if form == wm.FORM_U:
                case(tag('first element 256 more'), k, form, method, [('patch', at + 30, '01')])
                case(tag('first element with a high byte'), k, form, method, [('patch', at, '01')])
                case(tag('last element 256 more'), k, form, method, [('patch', at + 32 * (n - 1) + 30, '01')])
                case(tag('last element with byte 15 set'), k, form, method, [('patch', at + 32 * (n - 1) + 15, '40')])
                case(tag('last element with byte 16 set'), k, form, method, [('patch', at + 32 * (n - 1) + 16, '02')])
            else:
                case(tag('first padding byte set'), k, form, method, [('patch', at + n, '01')])
                case(tag('last padding byte set'), k, form, method, [('patch', len(cd) - 1, '80')])
            case(tag('last byte missing'), k, form, method, [('truncate', len(cd) - 1)])
            case(tag('one trailing byte'), k, form, method, [('append', '00')])
            case(tag('last word missing'), k, form, method, [('truncate', len(cd) - 32)])
            case(tag('one trailing word'), k, form, method, [('append', '00' * 32)])
            for cut in (0, 3, 4, 35, 36, 68, 99, 100, 131, 132):
                case(tag('cut to %d bytes' % cut), k, form, method, [('truncate', cut)])
        # a uint8[] element above 255 on either side of byte 260, in a set seal and in a Groth16-route seal; padding behind a set seal
        for k in (long_s, long_k):
            it = items[k]
            cd = swm.calldata_of(it, form, method)
            _, _, _, at, n = wm.parse_header(cd)
            if form == wm.FORM_U:
                for e in (4, 131, 259, 260, 261, n - 1):
                    case('element %d of %d is 256 more' % (e, n), k, form, method, [('patch', at + 32 * e + 30, '01')])
            else:
                case('first padding byte set', k, form, method, [('patch', at + n, '01')])
                case('last padding byte set', k, form, method, [('patch', len(cd) - 1, '01')])
    head = dict(note='eth_call requests to a RISC Zero router with a set route (one built-in route with the real proof\'s parameters, two keyed '
                     'trapdoor routes -- risc0_router_model.Key(seed) --, the set route of set_id) and the answers of '
                     'tests/risc0_router_set_wire_model.py with submitted_roots submitted first; parity unpinned: the reference holds no router and '
                     'no set verifier.  A verifyIntegrity call carries the claim digest of its item\'s image id and journal digest, or the item\'s '
                     'claim_digest where it has one.  An item with `base` is that item with byte edits of its seal (and its inputs unless it names its own).  One item and one case per line, a case as the values of case_fields; risc0_router_set_wire_model.load_fixture adds every case\'s '
                     'name and calldata.  Generated by make_risc0_router_set_wire_cases.py.',
                builtin=dict(control_root=real['control_root'], bn254_control_id=real['bn254_control_id']), key_seeds=list(KEY_SEEDS), set_id=SET_ID.hex(),
                set_selector=srouter.set_selector.hex(), route_selectors=[s.hex() for s in srouter.selectors],
                submitted_roots=[dict(root=r.hex(), seal=s.hex()) for r, s in stored], case_fields=list(cases[0]))
    dump = lambda v: json.dumps(v, separators=(',', ':'))
    rows = lambda v: '[\n' + ',\n'.join(dump(x) for x in v) + '\n]'
    path_out = os.path.join(HERE, 'risc0_router_set_wire_cases.json')
    with open(path_out, 'w') as f:
        f.write('{' + ',\n'.join('%s:%s' % (dump(k), dump(v)) for k, v in head.items()) + ',\n"items":' + rows(packed) + ',\n"cases":' + rows([list(c.values()) for c in cases]) + '}\n')
    json.load(open(path_out))
    print('%d items, %d cases, %d bytes' % (len(items), len(cases), os.path.getsize(path_out)))
    print(sorted(collections.Counter((c['status'], c['column']) for c in cases).items()))


if __name__ == '__main__':
    main()
