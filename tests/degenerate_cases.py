"""TEST TOOLING -- VALID proofs that reach the point-at-infinity and zero-scalar branches of the verifiers, each with a sibling that
differs in one value and must be rejected (a branch that accepts unconditionally, or computes garbage that happens to reject, fails
one of the two).  EIP-196/197 take the point at infinity everywhere, so a key or proof holding it is an ordinary input: a gnark circuit
without constant gates has Qk = O, one without multiplication gates Qm = O.

Groth16 (trapdoor keys of spec_model, discrete logs known): key points with chosen discrete logs (0 = O, equal / negated = equal /
opposite points), proofs with a chosen A or B scalar or a target C scalar, and signals chosen so that vk_x = O or vk_x = IC0.
PLONK (plonk_trapdoor_keys): keys with chosen discrete logs, proofs with chosen discrete logs / evaluations and the constructions
H_zeta = O, H_zeta_omega = O and linearised digest = O (the folded digest and both pairing inputs together are out of reach: see forge).
Every case asserts on the model side that it reaches its branch.  Everything is forged from fixed seeds."""
import functools
import hashlib
import random

import plonk_model as pm
import plonk_trapdoor_keys as T
import spec_model as m

R = m.R
VM = {'risc0': 0, 'sp1': 1}


# ---------------------------------------------------------------- Groth16
def _g1(k):
    p = m.g1_mul(m.G1_GEN, k % R)
    return (0, 0) if p is None else p


def _g2(k):
    return m.g2_words(m.g2_mul(m.G2_GEN, k % R))


def g16_key(rng, n_ic, over=None):
    """(vk dict, trapdoor) as spec_model.trapdoor_vk draws them, then `over` applied: {'alpha' | 'beta' | 'gamma' | 'delta' | 'ic<k>':
    int, or callable(drawn trapdoor) -> int}."""
    td = dict(alpha=rng.randrange(1, R), beta=rng.randrange(1, R), gamma=rng.randrange(1, R), delta=rng.randrange(1, R),
              ic=[rng.randrange(1, R) for _ in range(n_ic)])
    drawn = dict(td, ic=list(td['ic']))
    for k, v in (over or {}).items():
        v = (v(drawn) if callable(v) else v) % R
        if k.startswith('ic'):
            td['ic'][int(k[2:])] = v
        else:
            td[k] = v
    vk = dict(alpha1=_g1(td['alpha']), beta2=_g2(td['beta']), gamma2=_g2(td['gamma']), delta2=_g2(td['delta']),
              ic=[_g1(k) for k in td['ic']])
    return vk, td


def g16_prove(rng, td, signals, vm, a=None, b=None, c=None):
    """Scalars (a, b, c) of a valid proof: sgn a b + alpha beta + ell gamma + c delta = 0 (sgn = -1 for risc0, which negates A).  A given
    a or b is kept; a given c is a target, and a, b are solved for it.  Returns the scalars (the words follow from g16_words)."""
    sgn = -1 if vm == 'risc0' else 1
    ell = (td['ic'][0] + sum(s * k for s, k in zip(signals, td['ic'][1:]))) % R
    K = (td['alpha'] * td['beta'] + ell * td['gamma']) % R
    dl = td['delta']
    if c is None and dl:
        a = rng.randrange(1, R) if a is None else a
        b = rng.randrange(1, R) if b is None else b
        c = -(sgn * a * b + K) * pow(dl, -1, R) % R
        return a % R, b % R, c
    c = (rng.randrange(1, R) if c is None else c) % R      # delta = O: C multiplies nothing
    t = -(K + c * dl) % R                                   # sgn a b = t
    if a is None and b is None:
        a = rng.randrange(1, R)
    if a is not None and a % R:
        b = t * pow(sgn * a, -1, R) % R if b is None else b
    elif a is not None:
        assert t == 0, 'A = O needs the rest of the equation to vanish'
        b = rng.randrange(1, R) if b is None else b
    else:
        assert b % R, 'B = O with a target C: solve through a'
        a = t * pow(sgn * b, -1, R) % R
    return a % R, b % R, c


def g16_words(a, b, c):
    return m.proof_to_words(_g1(a), _g2(b), _g1(c))


def _sibling(td, a, b, c):
    """One value changed so that the equation breaks while the branch stays: C (if it is finite and delta is not O), else A (B finite)."""
    if td['delta'] and c:
        return a, b, (c + 1) % R
    assert b, 'no single value breaks this case'
    return (a + 1) % R, b, c


def _vkx_zero_signals(rng, td, n_sig):
    """Signals with ic0 + sum s_k ic_k = 0 (the last one solved; its IC must be finite)."""
    sig = [rng.randrange(R) for _ in range(n_sig - 1)]
    rest = (td['ic'][0] + sum(s * k for s, k in zip(sig, td['ic'][1:]))) % R
    return sig + [-rest * pow(td['ic'][n_sig], -1, R) % R]


def _g16_specs(n_ic_list, long_key):
    """(name, n_ic, vm, key overrides, signal rule, proof rule, branch)."""
    out = []
    vms = ('sp1', 'risc0')
    for j, n_ic in enumerate(n_ic_list):
        vm = vms[j % 2]
        other = vms[(j + 1) % 2]
        out += [('alpha = O', n_ic, vm, {'alpha': 0}, 'rand', {}, 'alpha'),
                ('beta2 = O', n_ic, other, {'beta': 0}, 'rand', {}, 'beta'),
                ('delta2 = O', n_ic, vm, {'delta': 0}, 'rand', {}, 'delta'),
                ('IC0 = O', n_ic, other, {'ic0': 0}, 'rand', {}, 'ic0')]
        if n_ic >= 2:
            out += [('IC1 = -IC0, vk_x = O', n_ic, vm, {'ic1': lambda td: -td['ic'][0]}, 'one0', {}, 'ic1neg'),
                    ('vk_x = O', n_ic, other, {}, 'vkx0', {}, 'vkx0')]
        if n_ic >= 3:
            out.append(('IC1 = IC2', n_ic, other, {'ic1': lambda td: td['ic'][2]}, 'rand', {}, 'ic12'))
        for v in vms:
            out += [('A = O', n_ic, v, {}, 'rand', {'a': 0}, 'A'),
                    ('C = O', n_ic, v, {}, 'rand', {'c': 0}, 'C')]
        out += [('B = O, A finite', n_ic, vm, {}, 'rand', {'b': 0}, 'B'),
                ('vk_x = IC0', n_ic, other, {}, 'zero', {}, 'vkxic0')]
    if long_key:                                           # n_ic = 129 tables are slow to build: two keys with overrides there
        out = [s for s in out if not s[3] or s[6] in (('ic0', 'ic1neg') if s[1] > 64 else ('alpha', 'ic0', 'ic1neg', 'ic12'))]
    return out


TRAPDOORS = {}                                             # key bytes -> trapdoor, for ordinary proofs beside the degenerate ones


@functools.lru_cache(maxsize=None)
def _ordinary_pool(vkb, vm):
    rng = random.Random(vkb + vm.encode())
    td = TRAPDOORS[vkb]
    out = []
    for _ in range(6):
        sig = [rng.randrange(R) for _ in range(len(td['ic']) - 1)]
        out.append((g16_words(*g16_prove(rng, td, sig, vm)), sig))
    return out


def ordinary_g16(vkb, vm, rng):
    """(proof words, signals) of an ordinary valid proof (random signals, A B C finite) for a key of groth16_cases: one of a small
    cached pool per key."""
    return rng.choice(_ordinary_pool(vkb, vm))


@functools.lru_cache(maxsize=None)
def _plonk_pool(vkb):
    vk = PLONK_KEYS[vkb]
    rng = T.rng_for('degenerate-plonk-ordinary', vkb)
    out = []
    for _ in range(4):
        pub = [rng.randrange(R) for _ in range(vk['nb_public'])]
        out.append((T.forge(vk, pub, rng), pub))
    return out


def ordinary_plonk_key(nb, nc):
    """A trapdoor key without degenerate points (for key sets beside the degenerate keys)."""
    vk = T.make_key(T.rng_for('degenerate-plonk-ordinary-key', nb, nc), nb, nc)
    PLONK_KEYS[T.vk_bytes(vk)] = vk
    return vk


def ordinary_plonk(vkb, rng):
    """(proof bytes, public inputs) of an ordinary valid proof for a key of plonk_cases (a small cached pool per key)."""
    return rng.choice(_plonk_pool(vkb))


def groth16_cases(n_ic_list=(1, 2, 3, 4, 5, 6), seed=0x6D67, long_key=False):
    """[(name, vm, vk dict, vk bytes, proof words, signals (ints), expected)] -- every valid case followed by its sibling."""
    out, plain = [], {}
    for name, n_ic, vm, over, srule, prule, branch in _g16_specs(n_ic_list, long_key):
        # cases without key overrides share their n_ic's plain key (one context, one set of tables)
        if over or n_ic not in plain:
            vk, td = g16_key(random.Random('%s/%d/%s' % (seed, n_ic, name if over else 'plain key')), n_ic, over)
            if not over:
                plain[n_ic] = vk, td
        vk, td = (vk, td) if over else plain[n_ic]
        rng = random.Random('%s/%d/%s/%s' % (seed, n_ic, vm, name))
        n_sig = n_ic - 1
        if srule == 'rand':
            sig = [rng.randrange(R) for _ in range(n_sig)]
        elif srule == 'zero':
            sig = [0] * n_sig
        elif srule == 'one0':                              # IC1 = -IC0, s1 = 1, the others 0: vk_x = O through a key point
            sig = [1] + [0] * (n_sig - 1)
        else:
            sig = _vkx_zero_signals(rng, td, n_sig)
        a, b, c = g16_prove(rng, td, sig, vm, **prule)
        vkx = m.compute_vk_x(vk, sig) if branch in ('ic1neg', 'vkx0', 'vkxic0') else None
        # ---- the case reaches its branch (model side)
        reach = {'alpha': vk['alpha1'] == (0, 0), 'beta': vk['beta2'] == ((0, 0), (0, 0)), 'delta': vk['delta2'] == ((0, 0), (0, 0)),
                 'ic0': vk['ic'][0] == (0, 0), 'ic1neg': n_ic >= 2 and vk['ic'][1] == m.g1_neg(vk['ic'][0]) and vkx is None,
                 'ic12': n_ic >= 3 and vk['ic'][1] == vk['ic'][2], 'vkx0': vkx is None, 'A': a == 0 and b != 0, 'B': b == 0 and a != 0,
                 'C': c == 0, 'vkxic0': vkx == (None if vk['ic'][0] == (0, 0) else vk['ic'][0]) and not any(sig)}[branch]
        assert reach, (name, n_ic)
        vkb = m.vk_to_words(vk)
        TRAPDOORS[vkb] = td
        tag = '%s %s n_ic=%d' % (name, vm, n_ic)
        out.append((tag, vm, vk, vkb, g16_words(a, b, c), sig, True))
        out.append((tag + ' / sibling', vm, vk, vkb, g16_words(*_sibling(td, a, b, c)), sig, False))
    return out


@functools.lru_cache(maxsize=None)
def short_cases():
    return groth16_cases()


@functools.lru_cache(maxsize=None)
def long_cases():
    return groth16_cases((9, 129), seed=0x6D68, long_key=True)


def g16_model(case):
    """(spec_model verdict, C-oracle verdict) of a Groth16 case."""
    import oracle_lib as ol
    name, vm, vk, vkb, words, sig, _ = case
    ints = [int.from_bytes(words[32 * i:32 * i + 32], 'big') for i in range(8)]
    a, b, c = (ints[0], ints[1]), ((ints[2], ints[3]), (ints[4], ints[5])), (ints[6], ints[7])
    return (m.groth16_verify(vm, vk, a, b, c, sig),
            ol.groth16_verify_vk(VM[vm], vkb, len(vk['ic']), words, [m.be32(s) for s in sig]))


# ---------------------------------------------------------------- PLONK
# (name, nb_public, n_c, key overrides, forge kwargs, branch) -- forge kwargs: over / evals / solve
_L = lambda dl: dl['L']
_NL = lambda dl: -dl['L']
PLONK_SPECS = [
    ('key Qk = Qm = O', 2, 0, {'qk': 0, 'qm': 0}, {}, 'key:qk,qm'),
    ('key Qk = Qm = O', 3, 1, {'qk': 0, 'qm': 0}, {}, 'key:qk,qm'),
    ('key Ql = Qr = Qo = S3 = O', 1, 0, {'ql': 0, 'qr': 0, 'qo': 0, 's3': 0}, {}, 'key:ql,qr,qo,s3'),
    ('key Ql = Qr = Qo = S3 = O', 8, 1, {'ql': 0, 'qr': 0, 'qo': 0, 's3': 0}, {}, 'key:ql,qr,qo,s3'),
    ('key Qcp = O', 2, 1, {'qcp': 0}, {}, 'key:qcp'),
    ('L = R = O = O', 2, 0, {}, {'over': {'L': 0, 'R': 0, 'O': 0}}, 'pt:L,R,O'),
    ('L = R = O = O', 0, 1, {}, {'over': {'L': 0, 'R': 0, 'O': 0}}, 'pt:L,R,O'),
    ('H0 = H1 = H2 = O', 3, 0, {}, {'over': {'H0': 0, 'H1': 0, 'H2': 0}}, 'pt:H0,H1,H2'),
    ('H0 = H1 = H2 = O', 2, 1, {}, {'over': {'H0': 0, 'H1': 0, 'H2': 0}}, 'pt:H0,H1,H2'),
    ('Z = O', 2, 0, {}, {'over': {'Z': 0}}, 'pt:Z'),
    ('Z = O', 8, 1, {}, {'over': {'Z': 0}}, 'pt:Z'),
    ('BSB22 = O', 2, 1, {}, {'over': {'BSB': 0}}, 'pt:BSB'),
    ('H_zeta_omega = O', 2, 0, {}, {'solve': 'hzw'}, 'hzw'),
    ('H_zeta_omega = O', 1, 1, {}, {'solve': 'hzw'}, 'hzw'),
    ('H_zeta = O', 2, 0, {}, {'solve': 'hz'}, 'hz'),
    ('H_zeta = O', 3, 1, {}, {'solve': 'hz'}, 'hz'),
    ('linearised digest = O', 2, 1, {}, {'solve': 'lin'}, 'lin'),
    ('linearised digest = O', 8, 1, {}, {'solve': 'lin'}, 'lin'),
    ('every evaluation 0', 2, 0, {}, {'evals': dict(l=0, r=0, o=0, s1=0, s2=0, zu=0)}, 'ev0'),
    ('every evaluation 0', 2, 1, {}, {'evals': dict(l=0, r=0, o=0, s1=0, s2=0, zu=0, qcpz=0)}, 'ev0'),
    ('evaluations 1 / R-1', 2, 1, {}, {'evals': dict(l=1, r=R - 1, o=1, s1=R - 1, s2=1, zu=R - 1, qcpz=1)}, 'ev1'),
    ('R = L', 2, 0, {}, {'over': {'R': _L}}, 'R=L'),
    ('R = -L', 3, 1, {}, {'over': {'R': _NL}}, 'R=-L'),
    ('Qk = O and Z = O and H_zeta = O', 2, 1, {'qk': 0}, {'over': {'Z': 0}, 'solve': 'hz'}, 'hz'),
]
_PW = {'L': 0, 'R': 2, 'O': 4, 'H0': 6, 'H1': 8, 'H2': 10, 'Z': 17, 'Hz': 20, 'Hzw': 22, 'BSB': 25}
_EW = {'l': 12, 'r': 13, 'o': 14, 's1': 15, 's2': 16, 'zu': 19, 'qcpz': 24}


def _w(proof, k):
    return int.from_bytes(proof[32 * k:32 * k + 32], 'big')


def _bump(proof, word):
    b = bytearray(proof)
    b[32 * word:32 * word + 32] = ((_w(proof, word) + 1) % R).to_bytes(32, 'big')
    return bytes(b)


def _neg(proof, word):
    b = bytearray(proof)
    b[32 * word + 32:32 * word + 64] = ((m.P - _w(proof, word + 1)) % m.P).to_bytes(32, 'big')
    return bytes(b)


PLONK_KEYS = {}                                           # key bytes -> trapdoor key


@functools.lru_cache(maxsize=None)
def plonk_key(nb, nc, over_items=()):
    over = dict(over_items)
    vk = T.make_key(T.rng_for('degenerate-plonk-key', nb, nc, tuple(sorted(over))), nb, nc, over=over)
    PLONK_KEYS[T.vk_bytes(vk)] = vk
    return vk


def _plonk_case(spec, seed, inputs=None):
    name, nb, nc, kover, fkw, branch = spec
    vk = plonk_key(nb, nc, tuple(sorted(kover.items())))
    pub = T.inputs(('degenerate', name, nb, nc, seed), nb) if inputs is None else inputs
    info = {}
    proof = T.forge(vk, pub, T.rng_for('degenerate-plonk-proof', name, nb, nc, seed), info=info, **fkw)
    # ---- the case reaches its branch (model and forger side)
    kind, _, what = branch.partition(':')
    if kind == 'key':
        assert all(vk['dlog'][k] == 0 and (vk[k] if k != 'qcp' else vk['qcp'][0]) == (0, 0) for k in what.split(',')), name
    elif kind == 'pt':
        assert all(_w(proof, _PW[k]) == _w(proof, _PW[k] + 1) == 0 for k in what.split(',')), name
    elif branch == 'hzw':
        assert info['hzw'] == 0 and _w(proof, 22) == _w(proof, 23) == 0, name
    elif branch == 'hz':
        assert info['hz'] == 0 and info['F'] == info['fe'] and _w(proof, 20) == _w(proof, 21) == 0, name
    elif branch == 'lin':
        assert info['f_lin'] == 0, name
    elif branch == 'ev0':
        assert all(info['evals'][k] == 0 for k in ('l', 'r', 'o', 's1', 's2', 'zu')), name
    elif branch == 'ev1':
        assert all(info['evals'][k] in (1, R - 1) for k in _EW), name
    elif branch == 'R=L':
        assert _w(proof, 2) == _w(proof, 0) and _w(proof, 3) == _w(proof, 1), name
    elif branch == 'R=-L':
        assert _w(proof, 2) == _w(proof, 0) and (_w(proof, 3) + _w(proof, 1)) % m.P == 0, name
    # the sibling: H_zeta_omega negated (the challenges and every branch above stay; the batched opening breaks), or where H_zeta_omega
    # is O, the claimed l(zeta) changed
    sib = _bump(proof, 12) if branch == 'hzw' else _neg(proof, 22)
    return vk, pub, proof, sib


@functools.lru_cache(maxsize=None)
def plonk_cases():
    """[(name, nb_public, n_c, trapdoor key, vk bytes, proof bytes, public inputs (ints), expected)]: valid case, then its sibling."""
    out = []
    for spec in PLONK_SPECS:
        name, nb, nc = spec[:3]
        vk, pub, proof, sib = _plonk_case(spec, 0)
        tag = '%s nb=%d n_c=%d' % (name, nb, nc)
        vkb = T.vk_bytes(vk)
        out.append((tag, nb, nc, vk, vkb, proof, pub, True))
        out.append((tag + ' / sibling', nb, nc, vk, vkb, sib, pub, False))
    return out


def plonk_model(case):
    """(plonk_model verdict, C-oracle verdict) of a PLONK case."""
    import oracle_lib as ol
    _, _, _, vk, vkb, proof, pub, _ = case
    return (T.model_verify(vk, proof, pub), ol.plonk_verify(vkb, T.pad27(proof), [x.to_bytes(32, 'big') for x in pub]))


# ---------------------------------------------------------------- SP1 PLONK (nb_public = 2, n_c = 1; inputs (vkey, sha256(pv) & (2^253 - 1)))
SP1_SPECS = [s for s in PLONK_SPECS if s[1] == 2 and s[2] == 1]


def sp1_verifier_hash(vkb):
    """A verifier hash per key (the gateway's routes need distinct selectors)."""
    return hashlib.sha256(b'degenerate sp1 plonk route' + vkb).digest()


@functools.lru_cache(maxsize=None)
def sp1_plonk_cases():
    """{key bytes: [(name, trapdoor key, program vkey, public values, proof bytes (selector + 27 words), expected)]} -- one SP1 PLONK
    context takes one key."""
    out = {}
    for spec in SP1_SPECS:
        name = spec[0]
        pv = hashlib.sha256(('pv ' + name).encode()).digest() * 3
        vkey = (int.from_bytes(hashlib.sha256(('vkey ' + name).encode()).digest(), 'big') % R).to_bytes(32, 'big')
        pub = [int.from_bytes(vkey, 'big'), m.sp1_hash_public_values(pv)]
        vk, _, proof, sib = _plonk_case(spec, 'sp1', inputs=pub)
        vkb = T.vk_bytes(vk)
        for tag, p, want in ((name, proof, True), (name + ' / sibling', sib, False)):
            out.setdefault(vkb, []).append((tag, vk, vkey, pv, sp1_verifier_hash(vkb)[:4] + p, want))
    return out


def sp1_model(vk, vkey, pv, proof):
    """(plonk_model status, C-oracle status) of an SP1 PLONK case."""
    import oracle_lib as ol
    vkb = T.vk_bytes(vk)
    return (pm.sp1_plonk_verify_proof(T.public_key_dict(vk), sp1_verifier_hash(vkb), vkey, pv, proof)[0],
            ol.sp1_plonk_verify_proof(vkb, sp1_verifier_hash(vkb), vkey, pv, proof)[0])
