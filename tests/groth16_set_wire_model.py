"""Python model of eth_call batches on a Groth16 key set of deployed contracts (include/zkv_groth16_set_wire.h):
the rules of the header in order, selectors from oracle_lib.keccak256, verdicts from oracle_lib.groth16_verify_vk.  Keys and proofs are
trapdoor ones with a fixed seed, as tests/test_groth16_key_sets_gpu.py::_parity_set makes them.  PARITY UNPINNED: the reference holds no
generic contract shell; the two forms are the Solidity verifiers snarkjs and gnark export."""
import random

import numpy as np

import oracle_lib as ol
import spec_model as m

FORM_SNARKJS, FORM_GNARK = 0, 1
SIGNATURES = {FORM_SNARKJS: 'verifyProof(uint256[2],uint256[2][2],uint256[2],uint256[%d])', FORM_GNARK: 'verifyProof(uint256[8],uint256[%d])'}
OK, FAILED, BAD_CALLDATA, NO_CONTRACT, NOT_IN_FIELD = 0, 1, 6, 9, 10
NO_KEY = 0xFFFFFFFF
VM = {'risc0': 0, 'sp1': 1}
P = m.P


def signature(form, n_signals):
    return SIGNATURES[form] % n_signals


def selector(form, n_signals):
    return ol.keccak256(signature(form, n_signals).encode())[:4]


PROOF_INVALID = ol.keccak256(b'ProofInvalid()')[:4]
NOT_IN_FIELD_ERROR = ol.keccak256(b'PublicInputNotInField()')[:4]


def encode(form, proof_words, signals):
    return selector(form, len(signals)) + bytes(proof_words) + b''.join(signals)


class Contracts:
    """keys: list of (vk_words, n_ic, vm 0 / 1, address, form)."""

    def __init__(self, keys):
        self.keys = list(keys)
        self.by_addr = {bytes(k[3]): j for j, k in enumerate(self.keys)}
        assert len(self.by_addr) == len(self.keys)
        self._verdicts = {}

    def table(self):
        """The sorted address table the library builds at creation: rows of (addr as five big-endian words, key, selector, n_sig)."""
        rows = []
        for j, (_, n_ic, _, addr, form) in enumerate(self.keys):
            sel, n_sig = (int.from_bytes(selector(form, n_ic - 1), 'big'), n_ic - 1) if n_ic > 1 else (0, NO_KEY)
            rows.append((bytes(addr), [int.from_bytes(addr[4 * k:4 * k + 4], 'big') for k in range(5)] + [j, sel, n_sig]))
        return np.array([r for _, r in sorted(rows)], dtype=np.uint32)

    def decode(self, to, cd):
        """Rules 2-4 on one request that lies inside the blob -> (verdict, resolved key, proof bytes, signals, some signal >= r)."""
        j = self.by_addr.get(bytes(to))
        if j is None:
            return NO_CONTRACT, NO_KEY, None, None, False
        _, n_ic, _, _, form = self.keys[j]
        n = n_ic - 1
        if n < 1 or len(cd) < 4 or cd[:4] != selector(form, n) or len(cd) != 4 + 32 * (8 + n):
            return BAD_CALLDATA, j, None, None, False
        sig = [cd[260 + 32 * b:292 + 32 * b] for b in range(n)]
        return 0, j, cd[4:260], sig, any(int.from_bytes(s, 'big') >= m.R for s in sig)

    def verify(self, j, proof, sig):
        key = (j, proof, b''.join(sig))
        if key not in self._verdicts:
            vk, n_ic, vm, _, _ = self.keys[j]
            self._verdicts[key] = ol.groth16_verify_vk(vm, vk, n_ic, proof, sig)
        return self._verdicts[key]

    def returndata(self, j, status):
        """(reverted, data) of a status under key j's form."""
        if status == NO_CONTRACT:
            return False, b''
        if status == BAD_CALLDATA:
            return True, b''
        if self.keys[j][4] == FORM_SNARKJS:
            return False, (1 if status == OK else 0).to_bytes(32, 'big')
        return (False, b'') if status == OK else (True, NOT_IN_FIELD_ERROR if status == NOT_IN_FIELD else PROOF_INVALID)

    def eth_call(self, to, cd):
        """One request inside the blob -> (status, resolved key, reverted, data)."""
        verdict, j, proof, sig, big = self.decode(to, cd)
        st = verdict if verdict else NOT_IN_FIELD if big else OK if self.verify(j, proof, sig) else FAILED
        return (st, j) + self.returndata(j, st)


def deployed_set(seed=2026):
    """About ten trapdoor keys: n_ic 1, 2, 3, 7, 17, 129, both forms, both vm_type conventions, one key with IC[1] off the curve, one key
    listed twice under two addresses (and two forms).  -> (keys as Contracts takes them, trapdoors)."""
    rng = random.Random(seed)
    keys, tds = [], []
    for j, n_ic in enumerate((1, 2, 3, 7, 17, 129, 2, 3)):
        vk, td = m.trapdoor_vk(rng, n_ic)
        keys.append([vk, n_ic, 'risc0' if j % 2 else 'sp1', (FORM_SNARKJS, FORM_GNARK)[(j // 2) % 2]]); tds.append(td)
    keys.append([keys[2][0], 3, keys[2][2], 1 - keys[2][3]]); tds.append(tds[2])                    # key 2 again, at another address, in the other form
    vk, td = m.trapdoor_vk(rng, 3)
    keys.append([dict(vk, ic=[vk['ic'][0], (vk['ic'][1][0], vk['ic'][1][1] ^ 1), vk['ic'][2]]), 3, 'sp1', FORM_GNARK]); tds.append(td)   # IC[1] off the curve
    out = []
    for vk, n_ic, vm, form in keys:
        out.append((m.vk_to_words(vk), n_ic, VM[vm], bytes(rng.randrange(256) for _ in range(20)), form))
    assert {(k[2], k[4]) for k in out} == {(a, b) for a in (0, 1) for b in (0, 1)}                  # every convention in every form
    return out, tds


def _other(addr, at):
    b = bytearray(addr); b[at] ^= 0x01
    return bytes(b)


def requests(keys, tds, seed=7):
    """The case list: per key the requests of the issue, each (class name, key, to, calldata)."""
    rng = random.Random(seed)
    out = []
    vm_name = {0: 'risc0', 1: 'sp1'}
    for j, ((vk, n_ic, vm, addr, form), td) in enumerate(zip(keys, tds)):
        n = n_ic - 1
        add = lambda name, cd, to=addr: out.append((name, j, to, bytes(cd)))
        sig = [rng.randrange(m.R) for _ in range(n)]
        if n:
            sig[0] = rng.choice([0, 1, m.R - 1, sig[0]])
        sb = [m.be32(s) for s in sig]
        words = m.proof_to_words(*m.trapdoor_prove(rng, td, sig, vm_name[vm]))
        sel = ol.keccak256(signature(form, n).encode())[:4]                  # (n = 0: the signature of a method no contract has)
        good = sel + words + b''.join(sb)
        add('valid', good)
        add('bytes_3', good[:3]); add('bytes_0', b'')
        add('addr_first', good, _other(addr, 0)); add('addr_last', good, _other(addr, 19))
        add('short_1', good[:-1]); add('long_1', good + b'\0')
        add('other_form', ol.keccak256(signature(1 - form, n).encode())[:4] + good[4:])
        if not n:
            continue
        bad = list(sb); bad[-1] = m.be32((sig[-1] + 1) % m.R)
        add('wrong_last_signal', sel + words + b''.join(bad))
        at = rng.randrange(n)
        eq_r = list(sb); eq_r[at] = m.be32(m.R)
        add('signal_r', sel + words + b''.join(eq_r))
        top = list(sb); top[n - 1 - at] = b'\xff' * 32
        add('signal_max', sel + words + b''.join(top))
        w = rng.choice([0, 1, 6, 7, 2, 5])                                   # a coordinate of A, C or B plus p (below 2^256)
        over = words[:32 * w] + m.be32(int.from_bytes(words[32 * w:32 * w + 32], 'big') + P) + words[32 * w + 32:]
        add('coordinate_ge_p', sel + over + b''.join(sb))
        add('other_convention', sel + m.proof_to_words(*m.trapdoor_prove(rng, td, sig, vm_name[1 - vm])) + b''.join(sb))
        for d in (-1, 1):                                                    # the right form's method of another contract size
            s2 = ol.keccak256(signature(form, n + d).encode())[:4]
            add('selector_n%+d' % d, s2 + good[4:])
            grown = good[4:] + bytes(32) if d > 0 else good[4:-32]
            add('call_n%+d' % d, s2 + grown)                                 # ... also with that method's own length
        add('bad_signal_bad_proof', sel + over[:32] + b'\xff' * 64 + over[96:] + b''.join(eq_r))
    return out


def expected(model, reqs):
    """[(status, resolved key, reverted, data)] of the case list."""
    return [model.eth_call(to, cd) for _, _, to, cd in reqs]


def check_coverage(keys, reqs, want):
    """Every status under both forms; per class the outcome the issue names; the model accepts and rejects within every verify class."""
    by = {}
    for (name, j, _, _), (st, rk, rev, data) in zip(reqs, want):
        by.setdefault(name, []).append((j, st))
        assert len(data) <= 96
    usable = [j for j, k in enumerate(keys) if k[1] > 1]
    broken = len(keys) - 1                                                   # the key with IC[1] off the curve fails every proof
    assert {st for j, st in by['valid']} == {OK, FAILED, BAD_CALLDATA}
    for j, st in by['valid']:
        assert st == (BAD_CALLDATA if keys[j][1] == 1 else FAILED if j == broken else OK), j
    for name in ('wrong_last_signal', 'coordinate_ge_p', 'other_convention'):
        assert sorted(j for j, _ in by[name]) == usable and {st for _, st in by[name]} == {FAILED}, name
    for name in ('signal_r', 'signal_max', 'bad_signal_bad_proof'):
        assert sorted(j for j, _ in by[name]) == usable and {st for _, st in by[name]} == {NOT_IN_FIELD}, name
    for name in ('bytes_3', 'bytes_0', 'short_1', 'long_1', 'other_form', 'selector_n-1', 'selector_n+1', 'call_n-1', 'call_n+1'):
        assert {st for _, st in by[name]} == {BAD_CALLDATA}, name
    for name in ('addr_first', 'addr_last'):
        assert len(by[name]) == len(keys) and {st for _, st in by[name]} == {NO_CONTRACT}, name
    for form in (FORM_SNARKJS, FORM_GNARK):
        seen = {st for (name, j, _, _), (st, _, _, _) in zip(reqs, want) if keys[j][4] == form}
        assert seen == {OK, FAILED, BAD_CALLDATA, NO_CONTRACT, NOT_IN_FIELD}, form
    assert {keys[j][2] for j, st in by['valid'] if st == OK} == {0, 1}       # a valid proof under either negation convention


def batch(reqs, want, n, seed, pick=None):
    """n requests drawn from the case list with repeats (or the requests `pick` names, n - 2 of them), shuffled, in one blob; from n = 3
    on two of them are no requests of the list: one whose offsets run past the blob and one whose offsets run backwards.  The requests
    start at every alignment: their lengths are odd and even.  -> (to bytes, blob, offsets uint64[n + 1], [(status, key, reverted, data)])."""
    rng = np.random.default_rng(seed)
    m_ = n - 2 if n >= 3 else n
    pick = rng.integers(0, len(reqs), m_) if pick is None else rng.permutation(pick)
    assert len(pick) == m_
    at = int(rng.integers(0, m_ + 1)) if n >= 3 else -1
    total = sum(len(reqs[j][3]) for j in pick)
    to, off, exp, blob = [], [0], [], []
    for r, j in enumerate(list(pick) + [None]):
        if r == at:
            off += [total + 1000, off[-1]]                                   # past the blob, then backwards to where the next one starts
            to += [reqs[0][2], reqs[0][2]]                                   # (a known address: the offsets alone decide)
            exp += [(BAD_CALLDATA, NO_KEY, True, b'')] * 2
        if j is None:
            break
        to.append(reqs[j][2]); blob.append(reqs[j][3]); off.append(off[-1] + len(reqs[j][3])); exp.append(want[j])
    assert len(to) == n and off[-1] == total
    return b''.join(to), b''.join(blob), np.array(off, dtype=np.uint64), exp


def counts(exp):
    """last_call_counts of a batch: placed, no contract, bad calldata, signal not in field."""
    st = [e[0] for e in exp]
    return [sum(s in (OK, FAILED) for s in st), st.count(NO_CONTRACT), st.count(BAD_CALLDATA), st.count(NOT_IN_FIELD)]
