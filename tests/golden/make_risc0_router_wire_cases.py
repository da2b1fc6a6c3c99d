#!/usr/bin/env python3
"""Generates tests/golden/risc0_router_wire_cases.json: named eth_call requests to a RISC Zero router with one built-in route (the real
proof's parameters, real_proofs.json) and two keyed trapdoor routes (risc0_router_model.Key), in the four call shapes -- two calldata
forms times verify / verifyIntegrity --, with the answers of tests/risc0_router_wire_model.py.  Every case is an item (seal, image id,
journal digest; a verifyIntegrity call carries the claim digest of the two), a form, a method and byte edits over the canonical call
(tests/wire_util.apply_ops).  PARITY UNPINNED BY CONSTRUCTION: the reference holds no router.

    python tests/golden/make_risc0_router_wire_cases.py
"""
import collections
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..', 'oracle'))
sys.path.insert(0, os.path.join(HERE, '..'))
import risc0_router_model as rm          # noqa: E402
import risc0_router_wire_model as wm     # noqa: E402
import spec_model as m                   # noqa: E402
from wire_util import apply_ops          # noqa: E402

H = bytes.fromhex
KEY_SEEDS = (0x5EA1, 0x5EA2)
LENGTHS = (0, 3, 4, 256, 257, 259, 260, 261, 292)


def in_a_of(it, method):
    """The first input of a call on item `it`: the image id, or (verifyIntegrity) the claim digest of image id and journal digest."""
    a, b = H(it['image_id']), H(it['journal_digest'])
    return a if method == wm.VERIFY else m.receipt_claim_ok_digest(a, b)


def calldata_of(it, form, method, ops=()):
    return apply_ops(wm.encode(form, method, H(it['seal']), in_a_of(it, method), H(it['journal_digest']) if method == wm.VERIFY else None), ops)


def main():
    real = json.load(open(os.path.join(HERE, 'real_proofs.json')))['risc0']
    rng = random.Random(0x7A7E7175)
    keys = [rm.Key(s) for s in KEY_SEEDS]
    router = wm.WireRouter(rm.Router([(H(real['control_root']), H(real['bn254_control_id']))], [k.triple() for k in keys]))
    seal, iid, jd = H(real['seal']), H(real['image_id']), H(real['journal_digest'])
    items = []

    def item(name, s, a, b):
        items.append(dict(name=name, seal=bytes(s).hex(), image_id=bytes(a).hex(), journal_digest=bytes(b).hex()))
        return len(items) - 1

    g_real = item('built-in route, real proof', seal, iid, jd)
    keyed = []
    for k, key in enumerate(keys):
        a = bytes(rng.randrange(256) for _ in range(32)); b = bytes(rng.randrange(256) for _ in range(32))
        keyed.append(item('keyed route %d, valid' % k, key.prove(a, b), a, b))
    for n in LENGTHS:
        if n != 260:
            item('built-in route, seal of %d bytes' % n, (seal + bytes(32))[:n], iid, jd)
    k0 = items[keyed[0]]
    for n in (259, 261, 292):
        item('keyed route 0, seal of %d bytes' % n, (H(k0['seal']) + bytes(32))[:n], H(k0['image_id']), H(k0['journal_digest']))
    item('unknown selector, real body', bytes(rng.randrange(256) for _ in range(4)) + seal[4:], iid, jd)
    item('unknown selector, 4 bytes', b'\xde\xad\xbe\xef', iid, jd)
    item('built-in route, bit flipped in C.x', seal[:4 + 192 + 31] + bytes([seal[4 + 192 + 31] ^ 1]) + seal[4 + 192 + 32:], iid, jd)
    item('built-in route, other journal digest', seal, iid, jd[:-1] + bytes([jd[-1] ^ 1]))
    item('keyed route 1, other image id', H(items[keyed[1]]['seal']), bytes(32), H(items[keyed[1]]['journal_digest']))
    item('keyed route 0 proof under keyed route 1 selector', keys[1].selector + H(k0['seal'])[4:], H(k0['image_id']), H(k0['journal_digest']))
    by_name = {it['name']: k for k, it in enumerate(items)}
    long_b, long_k = by_name['built-in route, seal of 261 bytes'], by_name['keyed route 0, seal of 292 bytes']

    cases = []

    def case(name, k, form, method, ops=()):
        cd = calldata_of(items[k], form, method, ops)
        rev, data, st, rv, col, kind = router.eth_call(cd)
        cases.append(dict(name='%s%s: %s' % ('UB'[form], 'vi'[method], name), form=form, method=method, item=k, ops=[list(o) for o in ops],
                          calldata_len=len(cd), reverted=int(rev), returndata=data.hex(), status=st, received=rv.hex(), column=col, kind=kind))

    word = lambda v: int(v).to_bytes(32, 'big').hex()
    sel = lambda sig: wm.selector_of(sig).hex()
    for form in (wm.FORM_U, wm.FORM_B):
        for method in (wm.VERIFY, wm.INTEGRITY):
            for k, it in enumerate(items):
                case(it['name'], k, form, method)
            for k in (g_real, keyed[0]):                     # every malformation on its own, over a call that verifies
                it = items[k]
                cd = calldata_of(it, form, method)
                _, _, a_at, at, n = wm.parse_header(cd)
                l_at = at - 32
                tag = lambda t: '%s [%s]' % (t, it['name'])
                case(tag('unknown function selector'), k, form, method, [('patch', 0, 'deadbeef')])
                case(tag("the other form's selector"), k, form, method, [('patch', 0, wm.selector(1 - form, method).hex())])
                case(tag("the other method's selector"), k, form, method, [('patch', 0, wm.selector(form, 1 - method).hex())])
                first = int.from_bytes(cd[4:36], 'big')
                case(tag('offset 32 more'), k, form, method, [('patch', 4, word(first + 32))])
                case(tag('offset 32 less'), k, form, method, [('patch', 4, word(first - 32))])
                case(tag('offset with a high byte'), k, form, method, [('patch', 4, '01')])
                case(tag('offset + 2^64'), k, form, method, [('patch', 4 + 23, '01')])
                if form == wm.FORM_B and method == wm.INTEGRITY:
                    case(tag('seal offset in the tuple 0x60'), k, form, method, [('patch', 36, word(0x60))])
                    case(tag('seal offset in the tuple 0x20'), k, form, method, [('patch', 36, word(0x20))])
                    case(tag('seal offset in the tuple + 2^32'), k, form, method, [('patch', 36 + 27, '01')])
                case(tag('length + 2^32'), k, form, method, [('patch', l_at + 27, '01')])
                case(tag('length + 2^64'), k, form, method, [('patch', l_at + 23, '01')])
                case(tag('length + 2^255'), k, form, method, [('patch', l_at, '80')])
                step = 1 if form == wm.FORM_U else 32
                case(tag('length more than present'), k, form, method, [('patch', l_at, word(n + step))])
                case(tag('length less than present'), k, form, method, [('patch', l_at, word(n - step))])
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
            # what lies behind the 260 bytes any route reads is still checked
            for k in (long_b, long_k):
                it = items[k]
                cd = calldata_of(it, form, method)
                _, _, _, at, n = wm.parse_header(cd)
                if form == wm.FORM_U:
                    case('element %d of %d is 256 more [%s]' % (n - 1, n, it['name']), k, form, method, [('patch', at + 32 * (n - 1) + 30, '01')])
                else:
                    case('first padding byte set [%s]' % it['name'], k, form, method, [('patch', at + n, '01')])
                    case('last padding byte set [%s]' % it['name'], k, form, method, [('patch', len(cd) - 1, '01')])
            # methods the router has and this layer does not simulate, and the single verifier's getters
            for sig, words in ((b'getVerifier(bytes4)', 1), (b'addVerifier(bytes4,address)', 2), (b'removeVerifier(bytes4)', 1), (b'getSelector()', 0),
                               (b'isInitialized()', 0)):
                case('%s' % sig.decode(), g_real, form, method, [('patch', 0, sel(sig)), ('truncate', 4 + 32 * words)])
    out = dict(note='eth_call requests to a RISC Zero router (one built-in route with the real proof\'s parameters, two keyed trapdoor routes) and the '
                    'answers of tests/risc0_router_wire_model.py; parity unpinned: the reference holds no router.  A verifyIntegrity call carries '
                    'the claim digest of its item\'s image id and journal digest.  Generated by make_risc0_router_wire_cases.py.',
               builtin=dict(control_root=real['control_root'], bn254_control_id=real['bn254_control_id']), key_seeds=list(KEY_SEEDS),
               route_selectors=[s.hex() for s in router.selectors], items=items, cases=cases)
    path = os.path.join(HERE, 'risc0_router_wire_cases.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=0, separators=(',', ':'))
        f.write('\n')
    print('%d items, %d cases, %d bytes' % (len(items), len(cases), os.path.getsize(path)))
    print(sorted(collections.Counter((c['status'], c['column']) for c in cases).items()))


if __name__ == '__main__':
    main()
