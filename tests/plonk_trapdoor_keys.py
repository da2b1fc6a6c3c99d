"""TEST TOOLING -- trapdoor PLONK keys for any public-input count, and proofs forged for them (include/zkv_plonk_keys.h).

The verifier equation of oracle/plonk_model.plonk_verify only involves the discrete logs of the points: with every key point a known
multiple of G and [tau]_2 from a known tau, a proof for ANY public inputs follows from the transcript alone --
  1. pick the discrete logs of L R O H0 H1 H2 Z (and the BSB22 commitment) and the claimed evaluations at random;
  2. run plonk_verify's transcript to gamma, beta, alpha, zeta, compute the linearised digest's and the folded digest's discrete logs
     F_lin, F and the folded evaluation fe, then lambda;
  3. set H_zeta = (F - fe) / (tau - zeta) G and H_zeta_omega = (z - zu) / (tau - zeta omega) G: both brackets of the batched check
        F + lambda z - (fe + lambda zu) + zeta h1 + lambda zeta omega h2 = tau (h1 + lambda h2)
     then hold for every lambda.
Keys and proofs use plonk_model's dict and word layouts; `proof_bytes` of a key without commitment (n_c = 0) is 24 words, and
`pad27` adds the three zero words both oracles expect (they read nothing past word 23 then, and zero words pass their range checks).
Parity unpinned by construction (the reference holds no PLONK code)."""
import hashlib
import random

import plonk_model as pm
import spec_model as m

R, P = m.R, m.P
be32, g1_bytes, finv = pm.be32, pm.g1_bytes, pm.finv


def _pt(k):
    return m.g1_mul(m.G1_GEN, k % R)


def make_key(rng, nb_public, n_c, log_n=None, cci=None, over=None):
    """A trapdoor key: dict in plonk_model's layout plus the discrete logs ('dlog') and tau.  `over` replaces discrete logs after the
    draws (so a key with overrides shares every other value with the key without): {name: int, or callable(dlog) -> int}; 0 gives the
    point at infinity, equal or negated discrete logs equal or opposite points."""
    if log_n is None:
        log_n = max(3, (nb_public + 2).bit_length() + 1)
    n = 1 << log_n
    w = pow(5, (R - 1) // n, R)
    assert pow(w, n, R) == 1 and pow(w, n // 2, R) != 1
    tau = rng.randrange(2, R)
    names = ('s1', 's2', 's3', 'ql', 'qr', 'qm', 'qo', 'qk') + (('qcp',) if n_c else ())
    dlog = {k: rng.randrange(1, R) for k in names}
    dlog.update(_resolve(over, dlog))
    if cci is None:
        cci = rng.randrange(0, n - nb_public) if n_c else 0
    vk = dict(size=n, size_inv=finv(n), generator=w, coset_shift=5, nb_public=nb_public, cci=[cci] if n_c else [],
              qcp=[pm.g1_wire(_pt(dlog['qcp']))] if n_c else [], g2=m.G2_GEN, g2_tau=m.g2_mul(m.G2_GEN, tau),
              **{k: pm.g1_wire(_pt(dlog[k])) for k in names if k != 'qcp'})
    vk['dlog'], vk['tau'] = dlog, tau
    return vk


def _resolve(over, dlog):
    """Overrides against the drawn discrete logs: every callable sees the values drawn, not other overrides."""
    return {k: (v(dlog) if callable(v) else v) % R for k, v in (over or {}).items()}


def proof_words(vk):
    return 24 + 3 * len(vk['qcp'])


def pad27(proof):
    return bytes(proof) + bytes(32 * 27 - len(proof))


def forge(vk, public_inputs, rng, over=None, evals=None, solve=None, info=None):
    """Proof bytes (24 + 3 n_c words) that plonk_verify accepts for `public_inputs` (ints < R) under the trapdoor key vk.

    Degenerate proofs (every override is applied after the same rng draws, so that the plain forgery does not change):
      over:  discrete logs of L R O H0 H1 H2 Z BSB ({name: int, or callable(drawn dlogs) -> int}; 0 = the point at infinity);
      evals: claimed evaluations l r o s1 s2 zu qcpz ({name: int});
      solve: 'hzw' -- H_zeta_omega = O: z(omega zeta) = dlog Z (zu is not hashed before zeta);
             'hz'  -- H_zeta = O: every claimed evaluation equals its digest's discrete log, and zu solves the affine equation
                      lin_eval(zu) = f_lin(zu), so that the folded digest equals [folded evaluation] G for every gamma_kzg;
             'lin' -- linearised digest = O (n_c = 1): qcp(zeta) solves f_lin = 0 (qcp(zeta) is hashed only after the digest).
      info:  a dict that receives the forger's intermediate values (f_lin, F, fe, hz / hzw discrete logs) for branch assertions.
    Out of reach, by design: the folded digest F at infinity (every free value is hashed into gamma_kzg, the challenge that
    multiplies it) and both pairing inputs D and Q at infinity together (the same, through lambda); these states are not forced."""
    n_c = len(vk['qcp'])
    d = vk['dlog']
    ks = ('s1', 's2', 's3', 'ql', 'qr', 'qm', 'qo', 'qk')
    dl = {k: rng.randrange(1, R) for k in ('L', 'R', 'O', 'H0', 'H1', 'H2', 'Z', 'BSB')}
    dl.update(_resolve(over, dl))
    pt = {k: _pt(v) for k, v in dl.items() if k != 'BSB' or n_c}
    l, r, o, s1, s2, zu = (rng.randrange(R) for _ in range(6))
    qcpz = rng.randrange(R) if n_c else 0
    ev = dict(l=l, r=r, o=o, s1=s1, s2=s2, zu=zu, qcpz=qcpz)
    ev.update({k: v % R for k, v in (evals or {}).items()})
    if solve == 'hzw':
        ev['zu'] = dl['Z']
    elif solve == 'hz':
        ev.update(l=dl['L'], r=dl['R'], o=dl['O'], s1=d['s1'], s2=d['s2'], qcpz=d['qcp'] if n_c else 0)
    elif solve == 'lin':
        assert n_c == 1, 'the linearised digest is solved through qcp(zeta)'
    elif solve is not None:
        raise ValueError(solve)
    l, r, o, s1, s2, zu, qcpz = (ev[k] for k in ('l', 'r', 'o', 's1', 's2', 'zu', 'qcpz'))
    # ---- challenges (plonk_verify)
    fs = pm.Transcript('gamma', 'beta', 'alpha', 'zeta')
    for k in ks:
        fs.add('gamma', g1_bytes(vk[k]))
    for q in vk['qcp']:
        fs.add('gamma', g1_bytes(q))
    for x in public_inputs:
        fs.add('gamma', be32(x))
    for k in ('L', 'R', 'O'):
        fs.add('gamma', g1_bytes(pt[k]))
    gamma = int.from_bytes(fs.challenge('gamma'), 'big') % R
    beta = int.from_bytes(fs.challenge('beta'), 'big') % R
    if n_c:
        fs.add('alpha', g1_bytes(pt['BSB']))
    fs.add('alpha', g1_bytes(pt['Z']))
    alpha = int.from_bytes(fs.challenge('alpha'), 'big') % R
    for k in ('H0', 'H1', 'H2'):
        fs.add('zeta', g1_bytes(pt[k]))
    zeta = int.from_bytes(fs.challenge('zeta'), 'big') % R
    # ---- public-input polynomial
    n, w, n_inv, u = vk['size'], vk['generator'], vk['size_inv'], vk['coset_shift']
    zh = (pow(zeta, n, R) - 1) % R
    lagrange0 = zh * finv(zeta - 1) % R * n_inv % R
    pi, acc = 0, 1
    for x in public_inputs:
        pi = (pi + zh * finv(zeta - acc) % R * n_inv % R * acc % R * x) % R
        acc = acc * w % R
    if n_c:
        wi = pow(w, vk['nb_public'] + vk['cci'][0], R)
        pi = (pi + zh * wi % R * finv(zeta - wi) % R * n_inv % R * pm.hash_to_field_bsb22(g1_bytes(pt['BSB']))) % R
    a2l0 = lagrange0 * alpha % R * alpha % R
    t1 = (l + beta * s1 + gamma) % R
    t2 = (r + beta * s2 + gamma) % R
    _s2 = -alpha * ((l + beta * zeta + gamma) % R) % R * ((r + beta * u % R * zeta + gamma) % R) % R * ((o + beta * u % R * u % R * zeta + gamma) % R) % R
    coeff_z = (a2l0 + _s2) % R
    zn2 = pow(zeta, n + 2, R)

    def linearised(zu, qcpz):                    # (lin_eval, f_lin): both affine in zu and qcpz
        lin_eval = -(pi - a2l0 + alpha * t1 % R * t2 % R * ((o + gamma) % R) % R * zu) % R
        _s1 = alpha * t1 % R * t2 % R * beta % R * zu % R
        terms = ([(qcpz, dl['BSB'])] if n_c else []) + [
            (l, d['ql']), (r, d['qr']), (l * r, d['qm']), (o, d['qo']), (1, d['qk']), (_s1, d['s3']), (coeff_z, dl['Z']),
            (-zh, dl['H0']), (-zn2 * zh, dl['H1']), (-zn2 * zn2 % R * zh, dl['H2'])]
        return lin_eval, sum(k * x for k, x in terms) % R

    if solve == 'hz':                            # lin_eval(zu) - f_lin(zu) = c0 + c1 zu = 0
        c0 = (linearised(0, qcpz)[0] - linearised(0, qcpz)[1]) % R
        c1 = (linearised(1, qcpz)[0] - linearised(1, qcpz)[1] - c0) % R
        zu = -c0 * finv(c1) % R
    elif solve == 'lin':                         # f_lin(qcpz) = k0 + k1 qcpz = 0
        k0 = linearised(zu, 0)[1]
        qcpz = -k0 * finv((linearised(zu, 1)[1] - k0) % R) % R
    lin_eval, f_lin = linearised(zu, qcpz)
    lin = _pt(f_lin)
    # ---- folding
    dig_dl = [f_lin, dl['L'], dl['R'], dl['O'], d['s1'], d['s2']] + ([d['qcp']] if n_c else [])
    digests = [lin, pt['L'], pt['R'], pt['O'], vk['s1'], vk['s2']] + list(vk['qcp'])
    values = [lin_eval, l, r, o, s1, s2] + ([qcpz] if n_c else [])
    fk = pm.Transcript('gamma')
    fk.add('gamma', be32(zeta))
    for g in digests:
        fk.add('gamma', g1_bytes(None if g is None or tuple(g) == (0, 0) else g))
    for v in values:
        fk.add('gamma', be32(v))
    fk.add('gamma', be32(zu))
    g_kzg = int.from_bytes(fk.challenge('gamma'), 'big') % R
    F = fe = 0
    gi = 1
    for x, v in zip(dig_dl, values):
        F, fe, gi = (F + gi * x) % R, (fe + gi * v) % R, gi * g_kzg % R
    tau, zeta_w = vk['tau'], zeta * w % R
    hz = _pt((F - fe) * finv(tau - zeta))
    hzw = _pt((dl['Z'] - zu) * finv(tau - zeta_w))
    if info is not None:
        info.update(f_lin=f_lin, F=F, fe=fe, hz=(F - fe) * finv(tau - zeta) % R, hzw=(dl['Z'] - zu) * finv(tau - zeta_w) % R, dlog=dict(dl),
                    evals=dict(l=l, r=r, o=o, s1=s1, s2=s2, zu=zu, qcpz=qcpz))
    wire = lambda p: be32(p[0]) + be32(p[1]) if p is not None else bytes(64)
    out = b''.join(wire(pt[k]) for k in ('L', 'R', 'O', 'H0', 'H1', 'H2'))
    out += b''.join(be32(v) for v in (l, r, o, s1, s2)) + wire(pt['Z']) + be32(zu) + wire(hz) + wire(hzw)
    if n_c:
        out += be32(qcpz) + wire(pt['BSB'])
    assert len(out) == 32 * proof_words(vk)
    return out


def public_key_dict(vk):
    """The key without its trapdoor (what plonk_model.vk_bytes and plonk_verify take)."""
    return {k: v for k, v in vk.items() if k not in ('dlog', 'tau')}


def vk_bytes(vk):
    return pm.vk_bytes(public_key_dict(vk))


def model_verify(vk, proof, public_inputs):
    return pm.plonk_verify(public_key_dict(vk), pad27(proof), list(public_inputs))


def seed_of(*parts):
    return int.from_bytes(hashlib.sha256(repr(parts).encode()).digest()[:8], 'big')


def rng_for(*parts):
    return random.Random(seed_of(*parts))


# ---------------------------------------------------------------- the committed fixture (tests/golden/plonk_keys_cases.json)
# The fixture stores only what is slow to recompute: the forged proofs, and per shape a verdict per case.  Keys come from their seeds
# (make_key, pinned by SHA-256), public inputs from SHA-256 of a tag (inputs), and every case is a named patch of its shape's valid
# proof, public inputs or key (case_names / apply_case).
import base64
import functools

SHAPES = [(nb, nc) for nb in (0, 1, 2, 3, 8, 9, 31, 64, 128) for nc in (0, 1)]
POOL_SHAPES = [(nb, nc) for nb in (0, 2, 9, 128) for nc in (0, 1)]
POOL_N = 4
_PT = {'L': 0, 'R': 2, 'H0': 6, 'H1': 8, 'Z': 17, 'Hz': 20, 'Hzw': 22, 'BSB': 25}
_KEY_PT = {'S1': 0, 'S3': 2, 'Ql': 3, 'Qk': 7, 'Qcp': 8}


@functools.lru_cache(maxsize=None)
def shape_key(nb, nc):
    return make_key(rng_for('plonk-keys-key', nb, nc), nb, nc)


def inputs(tag, nb):
    """nb public inputs < R, derived from a tag (the fixture does not store them)."""
    return [int.from_bytes(hashlib.sha256(('%r/%d' % (tag, i)).encode()).digest(), 'big') % R for i in range(nb)]


def valid_inputs(nb, nc):
    return inputs(('valid', nb, nc), nb)


def pool_inputs(nb, nc, j):
    return inputs(('pool', nb, nc, j), nb)


def forge_valid(nb, nc):
    return forge(shape_key(nb, nc), valid_inputs(nb, nc), rng_for('plonk-keys-valid', nb, nc))


def forge_pool(nb, nc, j):
    return forge(shape_key(nb, nc), pool_inputs(nb, nc, j), rng_for('plonk-keys-pool', nb, nc, j))


def case_names(nb, nc):
    """The cases of a shape, in fixture order: the valid proof, then tampered proofs, inputs and keys."""
    out = ['valid'] + ['pub%d+1' % i for i in range(nb)] + (['pub0=R', 'pub_last+R'] if nb else [])
    out += ['scalar%d+R' % w for w in (12, 13, 14, 15, 16, 19) + ((24,) if nc else ())] + ['eval_l+1']
    bsb = ('BSB',) if nc else ()
    out += ['%s.x+P' % p for p in ('L', 'Z', 'Hz') + bsb] + ['%s=inf' % p for p in ('L', 'H0', 'Z', 'Hz', 'Hzw') + bsb]
    out += ['-%s' % p for p in ('R', 'H1', 'Hzw') + bsb] + ['H0.y^1']
    out += ['key_S3_off_curve', 'key_Qk=inf', 'key_-Ql', 'key_S1.x+P', 'key_tau2_off_curve'] + (['key_Qcp_off_curve'] if nc else [])
    return out


def _get(b, w):
    return int.from_bytes(b[32 * w:32 * w + 32], 'big')


def _put(b, w, v):
    b[32 * w:32 * w + 32] = int(v).to_bytes(32, 'big')


def apply_case(name, vk, proof, pub):
    """(vk, proof, public inputs) of case `name` from the shape's valid triple (bytes, bytes, list of ints)."""
    vk, proof, pub = bytearray(vk), bytearray(proof), list(pub)
    kw = lambda p, c: 7 + 2 * _KEY_PT[p] + c                        # word of a key point's coordinate (c = 0: x, 1: y)
    if name.startswith('pub') and name.endswith('+1'):
        i = int(name[3:-2]); pub[i] = (pub[i] + 1) % R
    elif name == 'pub0=R':
        pub[0] = R
    elif name == 'pub_last+R':
        pub[-1] += R
    elif name.startswith('scalar'):
        w = int(name[6:-2]); _put(proof, w, _get(proof, w) + R)
    elif name == 'eval_l+1':
        _put(proof, 12, (_get(proof, 12) + 1) % R)
    elif name.endswith('.x+P') and not name.startswith('key'):
        w = _PT[name[:-4]]; _put(proof, w, _get(proof, w) + P)
    elif name.endswith('=inf') and not name.startswith('key'):
        w = _PT[name[:-4]]; _put(proof, w, 0); _put(proof, w + 1, 0)
    elif name.startswith('-'):
        w = _PT[name[1:]] + 1; _put(proof, w, (P - _get(proof, w)) % P)
    elif name == 'H0.y^1':
        _put(proof, 7, _get(proof, 7) ^ 1)
    elif name in ('key_S3_off_curve', 'key_Qcp_off_curve'):
        w = kw(name[4:].split('_')[0], 1); _put(vk, w, _get(vk, w) ^ 1)
    elif name == 'key_Qk=inf':
        _put(vk, kw('Qk', 0), 0); _put(vk, kw('Qk', 1), 0)
    elif name == 'key_-Ql':
        w = kw('Ql', 1); _put(vk, w, (P - _get(vk, w)) % P)
    elif name == 'key_S1.x+P':
        w = kw('S1', 0); _put(vk, w, _get(vk, w) + P)
    elif name == 'key_tau2_off_curve':
        w = (len(vk) - 128) // 32 + 1                              # [tau]_2 x_re (EIP-197 order x_im x_re y_im y_re)
        _put(vk, w, (_get(vk, w) + 1) % P)
    elif name != 'valid':
        raise ValueError(name)
    return bytes(vk), bytes(proof), pub


def parse_vk(vk):
    """plonk_model's key dict from key bytes (points as raw words, so that damaged keys stay as they are)."""
    w = [_get(vk, i) for i in range(len(vk) // 32)]
    nc = w[5]
    pt = lambda k: (w[7 + 2 * k], w[8 + 2 * k])
    g2 = lambda i: ((w[i + 1], w[i]), (w[i + 3], w[i + 2]))           # ((x_re, x_im), (y_re, y_im))
    g = 7 + 2 * (8 + nc)
    d = dict(size=w[0], size_inv=w[1], generator=w[2], coset_shift=w[3], nb_public=w[4], cci=[w[6]] if nc else [],
             qcp=[pt(8)] if nc else [], g2=g2(g), g2_tau=g2(g + 4))
    d.update({k: pt(i) for i, k in enumerate(('s1', 's2', 's3', 'ql', 'qr', 'qm', 'qo', 'qk'))})
    return d


def fixture_cases(shape):
    """(name, vk bytes, proof bytes, 32-byte public inputs, model verdict, C-oracle verdict or None) of every case of a fixture shape."""
    nb, nc = shape['nb_public'], shape['n_c']
    vk = vk_bytes(shape_key(nb, nc))
    assert hashlib.sha256(vk).hexdigest() == shape['vk_sha256'], 'trapdoor key derivation drifted from the fixture'
    proof = base64.b64decode(shape['proof'])
    names = case_names(nb, nc)
    assert len(names) == len(shape['model']) and (not shape['c_oracle'] or len(shape['c_oracle']) == len(names))
    for k, name in enumerate(names):
        v, p, q = apply_case(name, vk, proof, valid_inputs(nb, nc))
        yield name, v, p, [x.to_bytes(32, 'big') for x in q], int(shape['model'][k]), int(shape['c_oracle'][k]) if shape['c_oracle'] else None


def pool_arrays(entry):
    """A pool entry as (key bytes, proofs (POOL_N, proof_bytes), public inputs (POOL_N, nb_public, 32)) numpy arrays."""
    import numpy as np
    nb, nc = entry['nb_public'], entry['n_c']
    pb = 32 * (24 + 3 * nc)
    proofs = np.frombuffer(base64.b64decode(entry['proofs']), np.uint8).reshape(-1, pb)
    pub = np.frombuffer(b''.join(x.to_bytes(32, 'big') for j in range(len(proofs)) for x in pool_inputs(nb, nc, j)) or b'', np.uint8)
    return vk_bytes(shape_key(nb, nc)), proofs, pub.reshape(len(proofs), nb, 32)
