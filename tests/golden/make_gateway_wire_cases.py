#!/usr/bin/env python3
"""Generates tests/golden/gateway_wire_cases.json: named eth_call requests to an SP1 gateway with the Groth16 route and two PLONK routes
(the golden key of plonk_cases.json and the second trapdoor key of tests/test_sp1_gateway_gpu.py), in both calldata forms, with the
answers of tests/gateway_wire_model.py.  Every case is an item (vkey, public values, proof), a form and byte edits over the canonical
call (tests/wire_util.apply_ops).  PARITY UNPINNED BY CONSTRUCTION: the reference holds no gateway, no PLONK code and no router.

    python tests/golden/make_gateway_wire_cases.py
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..', 'oracle'))
sys.path.insert(0, os.path.join(HERE, '..'))
import gateway_wire_model as gwm      # noqa: E402
import plonk_model as pm              # noqa: E402
import spec_model as m                # noqa: E402
from wire_util import apply_ops       # noqa: E402

H = bytes.fromhex
PV_LENGTHS = (0, 1, 31, 32, 33, 96)


def main():
    load = lambda name: json.load(open(os.path.join(HERE, name)))
    real, plonk, corpus = load('real_proofs.json'), load('plonk_cases.json'), load('verify_corpus.json')
    rng = random.Random(0x6A7E7173)
    circ = pm.ToyCircuit(random.Random(0x6A7E5EED))
    vk1, vh1 = H(plonk['vk']), H(plonk['verifier_hash'])
    vk2, vh2 = pm.vk_bytes(circ.vk), b'\x5e\xc0\x4d\x02' + hashlib.sha256(b'second toy PLONK key').digest()[:28]
    gw = gwm.Gateway(True, [(vk1, vh1), (vk2, vh2)])

    def prove2(pv_len, tamper=None):
        vkey = int(rng.randrange(1 << 250)).to_bytes(32, 'big')
        pv = bytes(rng.randrange(256) for _ in range(pv_len))
        return vkey, pv, vh2[:4] + circ.prove(int.from_bytes(vkey, 'big'), m.sp1_hash_public_values(pv), tamper=tamper)

    s = real['sp1']
    sp1 = (H(s['vkey']), H(s['public_values']), H(s['proof']))
    named = lambda cases, name: next((H(c['vkey']), H(c['public_values']), H(c['proof'])) for c in cases if c.get('name') == name)
    p1 = named(plonk['cases'], 'valid, 96-byte public values')
    items = []

    def item(name, vkey, pv, proof):
        items.append(dict(name=name, vkey=vkey.hex(), pv=pv.hex(), proof=proof.hex()))
        return len(items) - 1

    for n in PV_LENGTHS:
        item('PLONK key 2, valid, public values %d bytes' % n, *prove2(n))
        if n != 96:
            item('Groth16 real proof, public values cut to %d bytes' % n, sp1[0], sp1[1][:n], sp1[2])
    g_real = item('Groth16 real proof', *sp1)
    for n in (0, 1, 2, 3, 4, 259, 261):
        item('Groth16 proof of %d bytes' % n, sp1[0], sp1[1], (sp1[2] + b'\0')[:n])
    for n in (867, 869):
        item('PLONK key 1 proof of %d bytes' % n, p1[0], p1[1], (p1[2] + b'\0')[:n])
    p1_long = len(items) - 1
    item('PLONK key 1, valid', *p1)
    item('PLONK key 1, valid, public values 200 bytes', *named(plonk['cases'], 'valid 1 (public values 200 bytes)'))
    item('PLONK key 1, word 0 (L.x) low bit flipped', *named(plonk['cases'], 'word 0 (L.x) low bit flipped'))
    item('PLONK key 1, public values changed', *named(plonk['cases'], 'public values changed'))
    sp1_cases = [c for c in corpus['cases'] if c['vm'] == 'sp1']
    for name in ('rerandomised 0', 'flip last public-values byte', 'flip bit in C.x', 'B out of subgroup', 'vkey >= R'):
        item('Groth16 ' + name, *named(sp1_cases, name))
    item('PLONK key 2, tampered (o5)', *prove2(96, tamper='o5'))
    v, w, p = prove2(96)
    item('PLONK key 2, wrong public values', v, w[:-1] + bytes([w[-1] ^ 1]), p)
    for k in range(2):
        item('unknown selector, %s body' % ('PLONK' if k else 'Groth16'), sp1[0], sp1[1], bytes(rng.randrange(256) for _ in range(4)) + (p1 if k else sp1)[2][4:])
    item('the RISC Zero selector', sp1[0], sp1[1], H(real['risc0']['seal']))
    item('Groth16 body under PLONK key 1 selector', sp1[0], sp1[1], vh1[:4] + sp1[2][4:])
    item('Groth16 body under PLONK key 2 selector', sp1[0], sp1[1], vh2[:4] + sp1[2][4:])
    item('PLONK key 1 proof under PLONK key 2 selector', p1[0], p1[1], vh2[:4] + p1[2][4:])
    item('PLONK key 1 proof under the Groth16 selector', p1[0], p1[1], sp1[2][:4] + p1[2][4:])
    p2_odd = next(k for k, it in enumerate(items) if it['name'] == 'PLONK key 2, valid, public values 33 bytes')

    cases = []

    def case(name, k, form, ops=()):
        it = items[k]
        cd = apply_ops(gwm.encode(form, H(it['vkey']), H(it['pv']), H(it['proof'])), ops)
        rev, data, st, rv, col = gw.eth_call(cd)
        cases.append(dict(name='%s: %s' % ('UB'[form], name), form=form, item=k, ops=[list(o) for o in ops], calldata_len=len(cd), reverted=int(rev),
                          returndata=data.hex(), status=st, received=rv.hex(), column=col))

    word = lambda v: int(v).to_bytes(32, 'big').hex()
    sel = lambda sig: gwm.selector_of(sig).hex()
    for form in (gwm.FORM_U, gwm.FORM_B):
        for k, it in enumerate(items):
            case(it['name'], k, form)
        for k in (g_real, p2_odd):                           # every malformation on its own, over a call that verifies
            it = items[k]
            cd = gwm.encode(form, H(it['vkey']), H(it['pv']), H(it['proof']))
            _, pv_at, pv_len, proof_at, proof_len = gwm.parse_header(cd)
            o2 = int.from_bytes(cd[68:100], 'big')
            tag = lambda t: '%s [%s]' % (t, it['name'])
            case(tag('unknown function selector'), k, form, [('patch', 0, 'deadbeef')])
            case(tag("the other form's selector"), k, form, [('patch', 0, gwm.selector(1 - form).hex())])
            case(tag('first offset 0x80'), k, form, [('patch', 36, word(0x80))])
            case(tag('first offset with a high byte'), k, form, [('patch', 36, '01')])
            case(tag('second offset 32 more'), k, form, [('patch', 68, word(o2 + 32))])
            case(tag('second offset 32 less'), k, form, [('patch', 68, word(o2 - 32))])
            case(tag('second offset + 2^64'), k, form, [('patch', 68 + 23, '01')])
            case(tag('public-values length + 2^32'), k, form, [('patch', 100 + 27, '01')])
            case(tag('public-values length + 2^255'), k, form, [('patch', 100, '80')])
            case(tag('proof length + 2^32'), k, form, [('patch', proof_at - 32 + 27, '01')])
            case(tag('proof length + 2^64'), k, form, [('patch', proof_at - 32 + 23, '01')])
            case(tag('proof length one more than present'), k, form, [('patch', proof_at - 32, word(proof_len + (1 if form == gwm.FORM_U else 32)))])
            case(tag('proof length one less than present'), k, form, [('patch', proof_at - 32, word(proof_len - (1 if form == gwm.FORM_U else 32)))])
            if form == gwm.FORM_U:
                case(tag('first public-values element 256 more'), k, form, [('patch', pv_at + 30, '01')])
                case(tag('last public-values element with a high byte'), k, form, [('patch', pv_at + 32 * (pv_len - 1), '01')])
                case(tag('first proof element 256 more'), k, form, [('patch', proof_at + 30, '01')])
                case(tag('last proof element with byte 15 set'), k, form, [('patch', proof_at + 32 * (proof_len - 1) + 15, '40')])
                case(tag('last proof element with byte 16 set'), k, form, [('patch', proof_at + 32 * (proof_len - 1) + 16, '02')])
            else:
                if pv_len % 32:
                    case(tag('first public-values padding byte set'), k, form, [('patch', pv_at + pv_len, '01')])
                    case(tag('last public-values padding byte set'), k, form, [('patch', proof_at - 33, '80')])
                case(tag('first proof padding byte set'), k, form, [('patch', proof_at + proof_len, '01')])
                case(tag('last proof padding byte set'), k, form, [('patch', len(cd) - 1, '01')])
            case(tag('last byte missing'), k, form, [('truncate', len(cd) - 1)])
            case(tag('one trailing byte'), k, form, [('append', '00')])
            case(tag('last word missing'), k, form, [('truncate', len(cd) - 32)])
            case(tag('one trailing word'), k, form, [('append', '00' * 32)])
            for n in (0, 3, 4, 36, 132, 163, proof_at - 32, proof_at):
                case(tag('cut to %d bytes' % n), k, form, [('truncate', n)])
        # a uint8[] element that is no byte, behind the 868 bytes any route reads
        if form == gwm.FORM_U:
            it = items[p1_long]
            h = gwm.parse_header(gwm.encode(form, H(it['vkey']), H(it['pv']), H(it['proof'])))
            case('proof element 868 of 869 is 256 more [%s]' % it['name'], p1_long, form, [('patch', h[3] + 32 * 868 + 30, '01')])
        # methods the gateway has and this layer does not simulate, and the single verifiers' getters
        for sig, words in ((b'routes(bytes4)', 1), (b'addRoute(address)', 1), (b'freezeRoute(bytes4)', 1), (b'verifierHash()', 0), (b'version()', 0), (b'VERIFIER_HASH()', 0)):
            case('%s' % sig.decode(), g_real, form, [('patch', 0, sel(sig)), ('truncate', 4 + 32 * words)])
    out = dict(note='eth_call requests to an SP1 gateway (Groth16 route, two PLONK routes) and the answers of tests/gateway_wire_model.py; '
                    'parity unpinned: the reference holds no gateway, no PLONK code and no router.  Generated by make_gateway_wire_cases.py.',
               routes=[dict(vk=vk1.hex(), verifier_hash=vh1.hex()), dict(vk=vk2.hex(), verifier_hash=vh2.hex())], items=items, cases=cases)
    path = os.path.join(HERE, 'gateway_wire_cases.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=0, separators=(',', ':'))
        f.write('\n')
    import collections
    print('%d items, %d cases, %d bytes' % (len(items), len(cases), os.path.getsize(path)))
    print(sorted(collections.Counter((c['status'], c['column']) for c in cases).items()))


if __name__ == '__main__':
    main()
