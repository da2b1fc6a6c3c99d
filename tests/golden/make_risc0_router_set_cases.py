#!/usr/bin/env python3
"""Generates tests/golden/risc0_router_set_cases.json: named seals to a RISC Zero router with a set route -- one built-in route (the real
proof's parameters, real_proofs.json), two keyed trapdoor routes (risc0_router_model.Key, so that a root proof exists for any root) and
the set route of a fixed set-builder image id -- with the answers of tests/risc0_router_set_model.py.  Every case is a seal, an image id
and a journal digest; a verify_integrity call carries the claim digest of the two and has the same answer.  The stored-root cases are
answered with `submitted_roots` submitted first.  PARITY UNPINNED BY CONSTRUCTION: the reference holds no router and no set verifier.

    python tests/golden/make_risc0_router_set_cases.py
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
import risc0_router_set_model as rsm     # noqa: E402
import set_inclusion_model as sm         # noqa: E402
import spec_model as m                   # noqa: E402

H = bytes.fromhex
KEY_SEEDS = (0x5E71, 0x5E72)
SET_ID = m.sha256(b'risc0 router set fixture: set builder image id')
DEPTHS = (0, 1, 2, 5, 20, 63, 64, 65)


def rand32(rng):
    return bytes(rng.randrange(256) for _ in range(32))


def claim_with_path(rng, depth):
    """(image id, journal digest, path, root) of a claim under a random path of `depth` siblings."""
    a, b = rand32(rng), rand32(rng)
    path = [rand32(rng) for _ in range(depth)]
    return a, b, path, sm.walk(m.receipt_claim_ok_digest(a, b), path)


def root_seal(key, root):
    """A valid seal of keyed route `key` for verify(seal, SET_ID, sha256(SET_ID || root))."""
    return key.prove(SET_ID, sm.root_journal(SET_ID, root))


def patch(seal, at, data):
    return seal[:at] + data + seal[at + len(data):]


def main():
    real = json.load(open(os.path.join(HERE, 'real_proofs.json')))['risc0']
    rng = random.Random(0x5E7C0DE5)
    keys = [rm.Key(s) for s in KEY_SEEDS]
    model = rsm.SetRouter(SET_ID, [(H(real['control_root']), H(real['bn254_control_id']))], [k.triple() for k in keys])
    rseal, iid, jd = H(real['seal']), H(real['image_id']), H(real['journal_digest'])
    word = lambda v: int(v).to_bytes(32, 'big')
    items = []

    def item(name, seal, a, b):
        items.append((name, bytes(seal), bytes(a), bytes(b)))

    # ---- Groth16 routes, unknown and short seals: as on a router without a set route
    item('built-in route, real proof', rseal, iid, jd)
    item('built-in route, other journal digest', rseal, iid, jd[:-1] + bytes([jd[-1] ^ 1]))
    for k, key in enumerate(keys):
        a, b = rand32(rng), rand32(rng)
        item('keyed route %d, valid' % k, key.prove(a, b), a, b)
        item('keyed route %d, 259 bytes' % k, key.prove(a, b)[:259], a, b)
    item('unknown selector', b'\xde\xad\xbe\xef' + rseal[4:], iid, jd)
    item('3 bytes', rseal[:3], iid, jd)
    item('empty seal', b'', iid, jd)
    item('set selector alone', model.set_selector, iid, jd)
    # ---- canonical set seals: every depth, both keyed routes as the root verifier
    stored = []
    for d in DEPTHS:
        for k, key in enumerate(keys):
            a, b, path, root = claim_with_path(rng, d)
            item('set seal, depth %d, root seal of keyed route %d' % (d, k), model.encode_seal(path, root_seal(key, root)), a, b)
    a, b, path, root = claim_with_path(rng, 3)
    good = model.encode_seal(path, root_seal(keys[0], root))
    item('set seal, other journal digest (another root than the seal proves)', good, a, b[:-1] + bytes([b[-1] ^ 1]))
    item('set seal, one sibling changed', patch(good, 4 + 128 + 32, rand32(rng)), a, b)
    item('set seal, root seal of the other keyed route under this selector', model.encode_seal(path, keys[1].selector + root_seal(keys[0], root)[4:]), a, b)
    item('set seal, root seal of the built-in route (the real proof: another claim)', model.encode_seal(path, rseal), a, b)
    item('set seal, root seal with an unknown selector', model.encode_seal(path, b'\xca\xfe\xf0\x0d' + root_seal(keys[0], root)[4:]), a, b)
    for n in (1, 3, 4, 259, 261, 292):
        item('set seal, root seal of %d bytes' % n, model.encode_seal(path, (root_seal(keys[0], root) + bytes(64))[:n]), a, b)
    item('set seal, nested: the root seal is a set seal', model.encode_seal(path, good), a, b)
    item('set seal, nested: the root seal is the set selector alone', model.encode_seal(path, model.set_selector), a, b)
    # ---- stored roots
    a2, b2, path2, root2 = claim_with_path(rng, 4)
    stored.append((root2, root_seal(keys[1], root2)))
    item('set seal, empty root seal, root submitted', model.encode_seal(path2, b''), a2, b2)
    item('set seal, empty root seal, depth 0, root not submitted', model.encode_seal([], b''), a2, b2)
    item('set seal, empty root seal, depth 65', model.encode_seal([rand32(rng) for _ in range(65)], b''), a2, b2)
    # ---- every edit of a header word or of the length, over the seal that verifies and over a seal with a 259-byte root seal (one padding byte:
    # a length of 260 then is canonical again, with another root seal)
    short = model.encode_seal(path, root_seal(keys[0], root)[:259])
    for tag, base in (('valid', good), ('259-byte root seal', short)):
        k = 3
        l_at = 4 + 128 + 32 * k
        ln = int.from_bytes(base[l_at:l_at + 32], 'big')
        t = lambda s: 'edited [%s]: %s' % (tag, s)
        item(t('first word 0x40'), patch(base, 4, word(0x40)), a, b)
        item(t('first word + 2^32'), patch(base, 4 + 27, b'\1'), a, b)
        item(t('path offset 0x60'), patch(base, 36, word(0x60)), a, b)
        item(t('path offset with a high byte'), patch(base, 36, b'\x80'), a, b)
        item(t('root seal offset 32 more'), patch(base, 68, word(0x60 + 32 * k + 32)), a, b)
        item(t('root seal offset 32 less'), patch(base, 68, word(0x60 + 32 * k - 32)), a, b)
        item(t('root seal offset + 2^64'), patch(base, 68 + 23, b'\1'), a, b)
        item(t('path length one more'), patch(base, 100, word(k + 1)), a, b)
        item(t('path length one less'), patch(base, 100, word(k - 1)), a, b)
        item(t('path length + 2^32'), patch(base, 100 + 27, b'\1'), a, b)
        item(t('path length 2^59 (times 32 wraps)'), patch(base, 100, word(1 << 59)), a, b)
        item(t('root seal length one more'), patch(base, l_at, word(ln + 1)), a, b)
        item(t('root seal length 32 more'), patch(base, l_at, word(ln + 32)), a, b)
        item(t('root seal length 32 less'), patch(base, l_at, word(ln - 32)), a, b)
        item(t('root seal length + 2^32'), patch(base, l_at + 27, b'\1'), a, b)
        item(t('root seal length + 2^255'), patch(base, l_at, b'\x80'), a, b)
        item(t('last byte missing'), base[:-1], a, b)
        item(t('one trailing byte'), base + b'\0', a, b)
        item(t('last word missing'), base[:-32], a, b)
        item(t('one trailing word'), base + bytes(32), a, b)
        for cut in (4, 5, 35, 36, 100, 132, 163, 164, l_at, l_at + 31, l_at + 32):
            item(t('cut to %d bytes' % cut), base[:cut], a, b)
    item('malformed [259-byte root seal]: padding byte set', patch(short, len(short) - 1, b'\1'), a, b)
    item('malformed [root seal of 261 bytes]: first padding byte set',
         patch(model.encode_seal(path, root_seal(keys[0], root) + b'\7'), 4 + 128 + 32 * 3 + 32 + 261, b'\1'), a, b)
    item('malformed [root seal of 261 bytes]: last padding byte set', model.encode_seal(path, root_seal(keys[0], root) + b'\7')[:-1] + b'\x80', a, b)

    for root, seal in stored:
        assert model.submit_root(root, seal)[0] == rsm.OK
    cases = []
    for name, seal, a, b in items:
        st, rv = model.verify(seal, a, b)
        assert (st, rv) == model.verify_integrity(seal, m.receipt_claim_ok_digest(a, b)), name
        cases.append(dict(name=name, seal=seal.hex(), image_id=a.hex(), journal_digest=b.hex(), status=st, received=rv.hex(), route=model.route(seal)))
    out = dict(note='Seals to a RISC Zero router with a set route (one built-in route with the real proof\'s parameters, two keyed trapdoor routes -- '
                    'risc0_router_model.Key(seed), written out under keyed --, the set route of set_id) and the answers of tests/risc0_router_set_model.py with submitted_roots submitted first; parity unpinned: the '
                    'reference holds no router and no set verifier.  A verify_integrity call carries the claim digest of its case\'s image id and '
                    'journal digest and has the same answer.  Generated by make_risc0_router_set_cases.py.',
               builtin=dict(control_root=real['control_root'], bn254_control_id=real['bn254_control_id']), key_seeds=list(KEY_SEEDS),
               keyed=[dict(vk_words=k.words.hex(), control_root=k.control_root.hex(), bn254_control_id=k.control_id.hex()) for k in keys], set_id=SET_ID.hex(),
               set_selector=model.set_selector.hex(), route_selectors=[s.hex() for s in model.selectors],
               submitted_roots=[dict(root=r.hex(), seal=s.hex()) for r, s in stored], cases=cases)
    path_out = os.path.join(HERE, 'risc0_router_set_cases.json')
    with open(path_out, 'w') as f:
        json.dump(out, f, indent=0, separators=(',', ':'))
        f.write('\n')
    print('%d cases, %d bytes' % (len(cases), os.path.getsize(path_out)))
    print(sorted(collections.Counter((c['status'], c['route']) for c in cases).items()))


if __name__ == '__main__':
    main()
