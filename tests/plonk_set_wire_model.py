"""Python model of eth_call batches on a PLONK key set of deployed contracts (include/zkv_plonk_set_wire.h): the
rules of the header in order, on the bytes, with integer arithmetic alone -- no pairing runs here.  The selector and the Error(string)
selector come from oracle_lib.keccak256; the verdict of a placed request is the one tests/golden/plonk_keys_cases.json records for its
(key, proof, inputs) (oracle/plonk_model.py's), or 1 for a pool proof.  Keys are the trapdoor keys of tests/plonk_trapdoor_keys.py.
PARITY UNPINNED: the reference holds no PLONK code and no contract shell; the contract is gnark's Solidity PLONK verifier."""
import hashlib
import json
import os

import numpy as np

import oracle_lib as ol
import plonk_trapdoor_keys as T

HERE = os.path.dirname(os.path.abspath(__file__))
R, P = T.R, T.P
SIGNATURE = 'Verify(bytes,uint256[])'
OK, FAILED, INVALID_PROOF_DATA, BAD_CALLDATA, NO_CONTRACT, NOT_IN_FIELD = 0, 1, 4, 6, 9, 10
R_NONE, R_INPUT_COUNT, R_INPUT_RANGE, R_PROOF_SIZE, R_OPENING_RANGE, R_EC = range(6)
MESSAGES = {R_INPUT_COUNT: b'wrong number of public inputs', R_INPUT_RANGE: b'inputs are bigger than r', R_PROOF_SIZE: b'wrong proof size',
            R_OPENING_RANGE: b'openings bigger than r', R_EC: b'error ec operation'}
NO_KEY = 0xFFFFFFFF
STRIDE = 128
OPENINGS = (12, 13, 14, 15, 16, 19)                      # and word 24 with a commitment
POINTS = (0, 2, 4, 6, 8, 10, 17, 20, 22)                 # and word 25 with a commitment


def selector():
    return ol.keccak256(SIGNATURE.encode())[:4]


def error_selector():
    return ol.keccak256(b'Error(string)')[:4]


def word(v):
    return int(v).to_bytes(32, 'big')


def encode(proof, inputs, lp=None, n_in=None, o1=0x40, o2=None, sel=None):
    """Calldata of Verify(proof, inputs); lp / n_in / o1 / o2 / sel replace the length words, the offset words and the selector."""
    proof = bytes(proof)
    body = proof + bytes(-len(proof) % 32)
    return (selector() if sel is None else sel) + word(o1) + word(0x60 + len(body) if o2 is None else o2) + word(len(proof) if lp is None else lp) + body + \
        word(len(inputs) if n_in is None else n_in) + b''.join(inputs)


def error_data(reason):
    msg = MESSAGES[reason]
    return error_selector() + word(0x20) + word(len(msg)) + msg + bytes(-len(msg) % 32)


def returndata(status, reason):
    """(reverted, data) of a (status, reason) pair a deployed PLONK set reports."""
    if reason:
        assert status == (NOT_IN_FIELD if reason == R_INPUT_RANGE else INVALID_PROOF_DATA)
        return True, error_data(reason)
    return {NO_CONTRACT: (False, b''), BAD_CALLDATA: (True, b''), OK: (False, word(1)), FAILED: (False, word(0))}[status]


def parse(cd):
    """Rule 3: (proof bytes, input words) of the one canonical layout, None for anything else."""
    if len(cd) < 4 + 128 or cd[:4] != selector():
        return None
    w = lambda at: int.from_bytes(cd[at:at + 32], 'big')
    o1, o2, lp = w(4), w(36), w(68)
    if o1 != 0x40 or lp >= 1 << 32:
        return None
    span = (lp + 31) // 32 * 32
    if o2 != 0x60 + span or len(cd) < 132 + span:
        return None
    n = w(100 + span)
    if n >= 1 << 32 or len(cd) != 132 + span + 32 * n:
        return None
    return cd[100:100 + lp], [cd[132 + span + 32 * k:164 + span + 32 * k] for k in range(n)]


def on_curve_or_infinity(x, y):
    """A G1 point as the EC precompiles take it."""
    if x >= P or y >= P:
        return False
    return (x == 0 and y == 0) or (y * y - x * x * x - 3) % P == 0


def sanity(nb, n_c, proof, inputs):
    """Rules 4 and 5 -> reason (0: the request is placed)."""
    if len(inputs) != nb:
        return R_INPUT_COUNT
    if any(int.from_bytes(x, 'big') >= R for x in inputs):
        return R_INPUT_RANGE
    if len(proof) != 32 * (24 + 3 * n_c):
        return R_PROOF_SIZE
    w = lambda k: int.from_bytes(proof[32 * k:32 * k + 32], 'big')
    if any(w(k) >= R for k in OPENINGS + ((24,) if n_c else ())):
        return R_OPENING_RANGE
    if not all(on_curve_or_infinity(w(k), w(k + 1)) for k in POINTS + ((25,) if n_c else ())):
        return R_EC
    return R_NONE


def key_shape(vk):
    """(nb_public, n_c) of key bytes."""
    return int.from_bytes(vk[128:160], 'big'), int.from_bytes(vk[160:192], 'big')


class Contracts:
    """keys: list of (vk bytes, address)."""

    def __init__(self, keys):
        self.keys = list(keys)
        self.shapes = [key_shape(vk) for vk, _ in self.keys]
        self.by_addr = {bytes(a): j for j, (_, a) in enumerate(self.keys)}
        assert len(self.by_addr) == len(self.keys)

    def table(self):
        """The sorted address table the library builds at creation: rows of (addr as five big-endian words, key, nb, n_c)."""
        rows = [(bytes(a), [int.from_bytes(a[4 * k:4 * k + 4], 'big') for k in range(5)] + [j, self.shapes[j][0], self.shapes[j][1]])
                for j, (_, a) in enumerate(self.keys)]
        return np.array([r for _, r in sorted(rows)], dtype=np.uint32)

    def classify(self, to, cd):
        """Rules 2-5 on one request that lies inside the blob -> (verdict, resolved key, reason, proof bytes, input words)."""
        j = self.by_addr.get(bytes(to))
        if j is None:
            return NO_CONTRACT, NO_KEY, R_NONE, None, None
        args = parse(bytes(cd))
        if args is None:
            return BAD_CALLDATA, j, R_NONE, None, None
        return 0, j, sanity(*self.shapes[j], *args), args[0], args[1]

    def eth_call(self, to, cd, recorded):
        """One request inside the blob; recorded: the verdict on record should it be placed -> (status, reason, key, reverted, data)."""
        verdict, j, reason, _, _ = self.classify(to, cd)
        if verdict:
            st = verdict
        elif reason:
            st = NOT_IN_FIELD if reason == R_INPUT_RANGE else INVALID_PROOF_DATA
        else:
            assert recorded in (0, 1), 'a placed request needs a verdict on record'
            st = OK if recorded else FAILED
        return (st, reason, j) + returndata(st, reason)


def fixture():
    return json.load(open(os.path.join(HERE, 'golden', 'plonk_keys_cases.json')))


def address_of(vk):
    return hashlib.sha256(b'plonk contract ' + hashlib.sha256(vk).digest()).digest()[:20]


TAMPERED_SHAPE = (3, 1)                                  # the shape whose tampered keys are deployed too


def deployed_set(fx):
    """24 contracts: the 18 shape keys, then the six tampered keys of shape TAMPERED_SHAPE -> [(vk bytes, address)]."""
    keys = [T.vk_bytes(T.shape_key(nb, nc)) for nb, nc in T.SHAPES]
    sh = next(s for s in fx['shapes'] if (s['nb_public'], s['n_c']) == TAMPERED_SHAPE)
    for _, vk, _, _, _, _ in T.fixture_cases(sh):
        if vk not in keys:
            keys.append(vk)
    assert len(keys) == 24
    return [(vk, address_of(vk)) for vk in keys]


def _sampled(name, nb):
    """Of the pubN+1 cases a shape keeps the first, a middle one and the last."""
    if not (name.startswith('pub') and name.endswith('+1')):
        return True
    return int(name[3:-2]) in (0, nb // 2, nb - 1)


def _flip(addr, at):
    b = bytearray(addr); b[at] ^= 0x01
    return bytes(b)


def _patch(proof, w, v):
    return proof[:32 * w] + word(v) + proof[32 * w + 32:]


def requests(keys, fx):
    """The case list, each (class name, key, to, calldata, verdict on record or None): the fixture's cases on the deployed keys (the
    pubN+1 cases sampled), the pool proofs, and per shape key what only the wire can express."""
    index = {vk: j for j, (vk, _) in enumerate(keys)}
    out = []
    valid = {}
    for sh in fx['shapes']:
        nb = sh['nb_public']
        for name, vk, proof, pub, model, _ in T.fixture_cases(sh):
            if vk in index and _sampled(name, nb):
                j = index[vk]
                out.append(('fx_' + name, j, keys[j][1], encode(proof, pub), model))
                if name == 'valid':
                    valid[j] = (proof, pub)
    for e in fx['pool']:
        vk, proofs, pub = T.pool_arrays(e)
        for k in range(len(proofs)):
            out.append(('pool', index[vk], keys[index[vk]][1], encode(proofs[k].tobytes(), [pub[k, b].tobytes() for b in range(pub.shape[1])]), 1))
    for j in sorted(valid):
        proof, pub = valid[j]
        addr = keys[j][1]
        nb, nc = key_shape(keys[j][0])
        good = encode(proof, pub)
        add = lambda name, cd, to=addr: out.append((name, j, to, bytes(cd), None))
        add('count+1', encode(proof, pub + [bytes(32)]))
        if nb:
            add('count-1', encode(proof, pub[:-1]))
        if nb == 1:
            add('count=0', encode(proof, []))
        other = proof + bytes(96) if nc == 0 else proof[:768]            # the other n_c's proof size
        add('lp_other_nc', encode(other, pub))
        add('lp=0', encode(b'', pub))
        add('lp=767', encode(proof[:767], pub)); add('lp=769', encode(proof[:768] + b'\x01', pub))
        span = len(proof)
        swapped = selector() + word(0x40 + 32 * len(pub)) + word(0x40) + word(len(pub)) + b''.join(pub) + word(len(proof)) + proof
        assert len(swapped) == len(good)
        add('swapped_arguments', swapped)
        for k, at in enumerate((4, 36, 68, 100 + span)):                 # a set high byte in each head word
            for byte in (0, 23):
                cd = bytearray(good); cd[at + byte] |= 0x80
                add('high_byte_word%d' % k, cd)
        add('n=2^32-1', encode(proof, pub, n_in=(1 << 32) - 1))
        add('lp=2^32-1', encode(proof, pub, lp=(1 << 32) - 1))
        add('short_1', good[:-1]); add('long_1', good + b'\0')
        add('bytes_3', good[:3]); add('bytes_0', b''); add('head_only', good[:131])
        add('other_selector', encode(proof, pub, sel=ol.keccak256(b'Verify(bytes,uint256[1])')[:4]))
        add('addr_first', good, _flip(addr, 0)); add('addr_last', good, _flip(addr, 19))
        # precedence: the earlier rule wins
        opening = _patch(proof, 12, int.from_bytes(proof[384:416], 'big') + R)
        add('size+opening', encode(_patch(other, 12, int.from_bytes(proof[384:416], 'big') + R), pub))
        add('opening+curve', encode(_patch(opening, 1, int.from_bytes(proof[32:64], 'big') ^ 1), pub))
        if nb:
            big = pub[:-1] + [word(R)]
            add('count+input', encode(proof, big + [bytes(32)]))
            add('input+size', encode(other, big))
            add('input+opening+curve', encode(_patch(opening, 1, int.from_bytes(proof[32:64], 'big') ^ 1), [word((1 << 256) - 1)] + pub[1:]))
    return out


WIRE_CLASSES = {
    'count+1': R_INPUT_COUNT, 'count-1': R_INPUT_COUNT, 'count=0': R_INPUT_COUNT, 'count+input': R_INPUT_COUNT,
    'input+size': R_INPUT_RANGE, 'input+opening+curve': R_INPUT_RANGE,
    'lp_other_nc': R_PROOF_SIZE, 'lp=0': R_PROOF_SIZE, 'lp=767': R_PROOF_SIZE, 'lp=769': R_PROOF_SIZE, 'size+opening': R_PROOF_SIZE,
    'opening+curve': R_OPENING_RANGE,
}
BAD_CLASSES = ('swapped_arguments', 'high_byte_word0', 'high_byte_word1', 'high_byte_word2', 'high_byte_word3', 'n=2^32-1', 'lp=2^32-1', 'short_1',
               'long_1', 'bytes_3', 'bytes_0', 'head_only', 'other_selector')


def expected(model, reqs):
    """[(status, reason, resolved key, reverted, data)] of the case list."""
    return [model.eth_call(to, cd, rec) for _, _, to, cd, rec in reqs]


def check_coverage(model, reqs, want):
    """Every status, every reason, both n_c, nb of 0 and of 128; per wire class the outcome the issue names; a request the rules leave
    unplaced has verdict 0 on record wherever one is on record."""
    by = {}
    for (name, j, _, _, rec), (st, rs, rk, rev, data) in zip(reqs, want):
        by.setdefault(name, []).append((j, st, rs))
        assert len(data) in (0, 32, 100) and len(data) <= STRIDE
        if st not in (OK, FAILED):
            assert not rec, name
    assert {st for v in by.values() for _, st, _ in v} == {OK, FAILED, INVALID_PROOF_DATA, BAD_CALLDATA, NO_CONTRACT, NOT_IN_FIELD}
    assert {rs for v in by.values() for _, _, rs in v} == set(range(6))
    for name, reason in WIRE_CLASSES.items():
        assert by[name] and {rs for _, _, rs in by[name]} == {reason}, name
    for name in BAD_CLASSES:
        assert by[name] and {(st, rs) for _, st, rs in by[name]} == {(BAD_CALLDATA, 0)}, name
    for name in ('addr_first', 'addr_last'):
        assert {(st, rs) for _, st, rs in by[name]} == {(NO_CONTRACT, 0)}, name
    placed = {(model.shapes[j], st) for v in by.values() for j, st, _ in v if st in (OK, FAILED)}
    for nb in (0, 128):
        for nc in (0, 1):
            assert {((nb, nc), OK), ((nb, nc), FAILED)} <= placed
    for reason in range(1, 6):
        assert {model.shapes[j][1] for v in by.values() for j, _, rs in v if rs == reason} == {0, 1}, reason
    assert {st for _, st, _ in by['fx_valid']} == {OK} and {st for _, st, _ in by['pool']} == {OK}
    tampered = [v for name, v in by.items() if name.startswith('fx_key_')]
    assert len(tampered) == 6 and all(v == [(v[0][0], FAILED, 0)] and v[0][0] >= 18 for v in tampered)       # an invalid key: placed, answers 0


def batch(reqs, want, n, seed, pick=None, shift=0):
    """n requests drawn from the case list with repeats (or the requests `pick` names, n - 2 of them), shuffled, in one blob that starts
    `shift` bytes into the buffer; from n = 3 on two of them are no requests of the list: one whose offsets run past the blob and one
    whose offsets run backwards.  -> (to bytes, blob, offsets uint64[n + 1], [(status, reason, key, reverted, data)])."""
    rng = np.random.default_rng(seed)
    m_ = n - 2 if n >= 3 else n
    pick = rng.integers(0, len(reqs), m_) if pick is None else rng.permutation(pick)
    assert len(pick) == m_
    at = int(rng.integers(0, m_ + 1)) if n >= 3 else -1
    total = shift + sum(len(reqs[j][3]) for j in pick)
    to, off, exp, blob = [], [shift], [], [bytes([0xA5]) * shift]
    for r, j in enumerate(list(pick) + [None]):
        if r == at:
            off += [total + 1000, off[-1]]                                   # past the blob, then backwards to where the next one starts
            to += [reqs[0][2], reqs[0][2]]                                   # (a known address: the offsets alone decide)
            exp += [(BAD_CALLDATA, R_NONE, NO_KEY, True, b'')] * 2
        if j is None:
            break
        to.append(reqs[j][2]); blob.append(reqs[j][3]); off.append(off[-1] + len(reqs[j][3])); exp.append(want[j])
    assert len(to) == n and off[-1] == total
    return b''.join(to), b''.join(blob), np.array(off, dtype=np.uint64), exp


def counts(exp):
    """last_call_counts of a batch: placed, no contract, bad calldata, reasons 1 .. 5."""
    st = [e[0] for e in exp]
    rs = [e[1] for e in exp]
    return [sum(s in (OK, FAILED) for s in st), st.count(NO_CONTRACT), st.count(BAD_CALLDATA)] + [rs.count(r) for r in range(1, 6)]
