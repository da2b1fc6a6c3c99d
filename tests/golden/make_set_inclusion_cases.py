#!/usr/bin/env python3
"""Generates tests/golden/set_inclusion_cases.json from tests/set_inclusion_model.py (fixed seed): the hash cases of the keccak-256 Merkle
path (known-answer vectors, leaves, nodes, every leaf's walk in trees of 1, 2, 3, 5, 8 and 21 leaves, walks of depth 20, 64 and 65) and
the batches -- about 200 claims over four trees behind a trapdoor key (n_ic = 6, RISC Zero convention: valid root proofs for arbitrary
roots), and a small batch behind the built-in RISC Zero key with the real proof of real_proofs.json as root seal.  Every status is the
model's; the distinct (seal, root) pairs are kept to about a dozen because each costs a pairing check in pure Python.
PARITY UNPINNED: the reference holds no set verifier.

    python tests/golden/make_set_inclusion_cases.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..', 'oracle'))
sys.path.insert(0, os.path.join(HERE, '..'))
import set_inclusion_model as sm      # noqa: E402
import spec_model as m                # noqa: E402

H = bytes.fromhex
TREES = (50, 47, 53, 50)              # claims per tree of the keyed batch: three behind valid root seals, the last behind a stored root
SEED = 0x5E71C1


def rand32(rng):
    return bytes(rng.randrange(256) for _ in range(32))


def hash_cases(rng, set_id):
    out = {'keccak': [{'msg': b.hex(), 'digest': m.keccak256(b).hex()} for b in (b'', b'abc', b'LEAF_TAG', bytes(range(135)))]}
    claims = [bytes(32), bytes([0xFF]) * 32, rand32(rng)]
    out['leaf'] = [{'claim': c.hex(), 'leaf': sm.leaf(c).hex()} for c in claims]
    a = rand32(rng)
    lo, hi = (a[:31] + b'\x00'), (a[:31] + b'\x01')                   # equal up to the last byte
    first = b'\x00' + a[1:]
    pairs = [('a<b', lo, hi), ('a>b', hi, lo), ('a==b', a, a), ('first byte decides', bytes([0x80]) + a[1:], first),
             ('high bit of a byte (unsigned compare)', a[:7] + b'\x7f' + a[8:], a[:7] + b'\x80' + a[8:])]
    out['node'] = [{'name': n, 'a': x.hex(), 'b': y.hex(), 'node': sm.node(x, y).hex()} for n, x, y in pairs]
    out['journal'] = [{'root': r.hex(), 'digest': sm.root_journal(set_id, r).hex()} for r in (bytes(32), rand32(rng))]
    walks = []
    for size in (1, 2, 3, 5, 8, 21):
        ids = [(rand32(rng), rand32(rng)) for _ in range(size)]
        digests = [m.receipt_claim_ok_digest(i, j) for i, j in ids]
        root, paths = sm.tree_paths([sm.leaf(d) for d in digests])
        for k in range(size):
            assert sm.walk(digests[k], paths[k]) == root
            walks.append({'name': 'tree%d/%d' % (size, k), 'image_id': ids[k][0].hex(), 'journal_digest': ids[k][1].hex(), 'claim': digests[k].hex(),
                          'path': b''.join(paths[k]).hex(), 'root': root.hex()})
    for depth in (20, 64, 65):
        i, j = rand32(rng), rand32(rng)
        d = m.receipt_claim_ok_digest(i, j)
        path = [rand32(rng) for _ in range(depth)]
        walks.append({'name': 'depth%d' % depth, 'image_id': i.hex(), 'journal_digest': j.hex(), 'claim': d.hex(), 'path': b''.join(path).hex(),
                      'root': sm.walk(d, path).hex()})
    out['walks'] = walks
    return out


def keyed_cases(rng, set_id):
    control_root, control_id = rand32(rng), (int.from_bytes(rand32(rng), 'big') % m.R).to_bytes(32, 'big')
    vk, td = m.trapdoor_vk(rng, 6)
    selector = H('5e71c1d0')
    inner = sm.KeyedRisc0Verifier(vk, selector, control_root, control_id)
    sv = sm.SetVerifier(inner, set_id)

    def prove(root):
        claim = m.receipt_claim_ok_digest(set_id, sm.root_journal(set_id, root))
        a, b, c = m.trapdoor_prove(rng, td, inner.signals(claim), 'risc0')
        return selector + m.proof_to_words(a, b, c)

    trees = []
    for size in TREES:
        ids = [(rand32(rng), rand32(rng)) for _ in range(size)]
        root, paths = sm.tree_paths([sm.leaf(m.receipt_claim_ok_digest(i, j)) for i, j in ids])
        trees.append((ids, paths, root))
    seals = [prove(t[2]) for t in trees]                              # seals[3] is submitted, not sent with the claims
    s0 = seals[0]
    ax = int.from_bytes(s0[4:36], 'big') + m.P
    assert ax < 1 << 256
    root_seals = seals[:3] + [b'\xde\xad\xbe\xef' + s0[4:],          # 3: spliced selector
                              s0[:4] + m.be32(ax) + s0[36:],          # 4: A.x >= q
                              s0[:-1]]                                # 5: 259 bytes
    claims = []

    def add(kind, t, k, idx, path=None):
        ids, paths, _ = trees[t]
        claims.append({'kind': kind, 'image_id': ids[k][0], 'journal_digest': ids[k][1], 'path': paths[k] if path is None else path, 'root_idx': idx})

    for t in range(4):
        ids, paths, _ = trees[t]
        idx = t if t < 3 else sm.STORED
        for k in range(len(ids)):
            if k == len(ids) // 2:                                    # one flipped sibling byte per tree: a straggler
                p = [bytes(s) for s in paths[k]]
                at = rng.randrange(len(p))
                p[at] = p[at][:5] + bytes([p[at][5] ^ 0x40]) + p[at][6:]
                add('straggler', t, k, idx, p)
            elif t == 0 and k == 7: add('wrong_seal', t, k, 1)
            elif t == 0 and k == 11: add('bad_selector', t, k, 3)
            elif t == 0 and k == 13: add('big_coordinate', t, k, 4)
            elif t == 1 and k == 5: add('short_seal', t, k, 5)
            elif t == 1 and k == 9: add('bad_index', t, k, len(root_seals))
            elif t == 2 and k == 3: add('deep', t, k, 2, [rand32(rng) for _ in range(65)])
            elif t == 2 and k == 4: add('depth64', t, k, 2, [rand32(rng) for _ in range(64)])      # the limit itself is hashed: a straggler
            else: add('honest', t, k, idx)
    out = []
    for c in claims:
        unsub = sv.verify(c['image_id'], c['journal_digest'], c['path'], c['root_idx'], root_seals)
        c['claim'] = m.receipt_claim_ok_digest(c['image_id'], c['journal_digest'])
        assert sv.verify_claim_digest(c['claim'], c['path'], c['root_idx'], root_seals) == unsub
        out.append((c, unsub))
    assert sv.submit_root(trees[0][2], seals[1])[0] == m.VERIFICATION_FAILED and not sv.roots      # (the wrong_seal pair's mirror image)
    assert sv.submit_root(trees[3][2], seals[3]) == (m.OK, None) and trees[3][2] in sv.roots
    rows = []
    for c, unsub in out:
        st, recv = sv.verify(c['image_id'], c['journal_digest'], c['path'], c['root_idx'], root_seals)
        assert (st, recv) == unsub or c['root_idx'] == sm.STORED
        rows.append({'kind': c['kind'], 'image_id': c['image_id'].hex(), 'journal_digest': c['journal_digest'].hex(), 'claim': c['claim'].hex(),
                     'path': b''.join(c['path']).hex(), 'root_idx': c['root_idx'], 'status': st, 'recv': (recv or bytes(4)).hex(),
                     'status_unsubmitted': unsub[0]})
    kinds = {}
    for r in rows:
        kinds.setdefault(r['kind'], set()).add(r['status'])
    assert kinds == {'honest': {m.OK}, 'straggler': {m.VERIFICATION_FAILED}, 'wrong_seal': {m.VERIFICATION_FAILED}, 'bad_selector': {m.SELECTOR_MISMATCH},
                     'big_coordinate': {m.VERIFICATION_FAILED}, 'short_seal': {m.INVALID_PROOF_DATA}, 'bad_index': {m.INVALID_PROOF_DATA},
                     'deep': {m.INVALID_PROOF_DATA}, 'depth64': {m.VERIFICATION_FAILED}}, kinds
    return {'control_root': control_root.hex(), 'bn254_control_id': control_id.hex(), 'vk_words': m.vk_to_words(vk).hex(), 'root_selector': selector.hex(),
            'root_seals': [s.hex() for s in root_seals],
            'stored': {'root': trees[3][2].hex(), 'seal': seals[3].hex(), 'rejected_root': trees[0][2].hex(), 'rejected_seal': seals[1].hex()},
            'claims': rows, 'model_pairings': sv.pairings}


def real_cases(rng, set_id, real):
    r = real['risc0']
    inner = sm.builtin_verifier(H(r['control_root']), H(r['bn254_control_id']))
    sv = sm.SetVerifier(inner, set_id)
    ids = [(rand32(rng), rand32(rng)) for _ in range(5)]
    _, paths = sm.tree_paths([sm.leaf(m.receipt_claim_ok_digest(i, j)) for i, j in ids])
    seal = H(r['seal'])
    spliced = b'\x01\x02\x03\x04' + seal[4:]
    rows = []
    for (i, j), p in zip(ids, paths):
        a, b = sv.verify(i, j, p, 0, [seal, spliced]), sv.verify(i, j, p, 1, [seal, spliced])
        assert a == (m.VERIFICATION_FAILED, None) and b == (m.SELECTOR_MISMATCH, spliced[:4])
        rows.append({'image_id': i.hex(), 'journal_digest': j.hex(), 'path': b''.join(p).hex()})
    return {'control_root': r['control_root'], 'bn254_control_id': r['bn254_control_id'], 'root_seals': [seal.hex(), spliced.hex()], 'claims': rows,
            'status': [m.VERIFICATION_FAILED, m.SELECTOR_MISMATCH], 'recv': [bytes(4).hex(), spliced[:4].hex()], 'model_pairings': sv.pairings}


def main():
    rng = random.Random(SEED)
    real = json.load(open(os.path.join(HERE, 'real_proofs.json')))
    set_id = rand32(rng)
    doc = {'note': 'written by make_set_inclusion_cases.py from tests/set_inclusion_model.py; parity unpinned',
           'set_builder_image_id': set_id.hex(), 'set_selector': sm.set_selector(set_id).hex(),
           'hash': hash_cases(rng, set_id), 'keyed': keyed_cases(rng, set_id), 'real': real_cases(rng, set_id, real)}
    with open(os.path.join(HERE, 'set_inclusion_cases.json'), 'w') as f:
        json.dump(doc, f, separators=(',', ':'))
        f.write('\n')
    print('claims: %d keyed, %d real; model pairings: %d + %d' % (len(doc['keyed']['claims']), len(doc['real']['claims']), doc['keyed']['model_pairings'],
                                                                   doc['real']['model_pairings']))


if __name__ == '__main__':
    main()
