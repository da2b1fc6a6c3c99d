"""Model of the RISC Zero verifier router (include/zkv_risc0_router.h): the routing rule in numpy (as gateway_model.routes), the selector
and key-digest derivation over key words written from risc0/crypto.rs:136-195 and risc0/verifier.rs:128-144 with Python integers and
hashlib, and the per-route verifiers -- spec_model.Risc0Verifier for a built-in-key route, set_inclusion_model.KeyedRisc0Verifier with the
derived selector for a keyed route -- with the pairing by the C oracle.  The per-slot front end the device runs before the pairing of a
keyed route (csrc/zkv_rzrouter_prep.h) is modelled too.  PARITY UNPINNED for the routing: the reference holds no router."""
import hashlib
import random

import numpy as np

import oracle_lib as ol
import set_inclusion_model as sm
import spec_model as m

SHORT, NOT_FOUND = -1, -2          # route codes besides 0 .. R - 1
OK, VERIFICATION_FAILED, INVALID_PROOF_DATA, SELECTOR_MISMATCH, ROUTE_NOT_FOUND = 0, 1, 4, 5, 8
FL_ALIVE, FL_A_INF, FL_B_INF, FL_C_INF = 1, 2, 4, 8
MAX_ROUTES, MAX_KEYED, KEY_BYTES = 32, 8, 832


def _sha(b):
    return hashlib.sha256(bytes(b)).digest()


# ---------------------------------------------------------------- derivation over key words (zkv_groth16_ctx_create's layout)
def tagged_struct(tag, down):
    """crypto.rs:112-134: sha256(sha256(tag) || down digests || u16 big-endian of (len << 8))."""
    return _sha(_sha(tag) + b''.join(down) + ((len(down) << 8) & 0xFFFF).to_bytes(2, 'big'))


def vk_digest_of_words(words, n_ic=6):
    """compute_verifier_key_digest (crypto.rs:136-195) over alpha (2 words) | beta, gamma, delta (4 each) | ic (2 each)."""
    words = bytes(words)
    assert len(words) == 448 + 64 * n_ic
    ic_list = bytes(32)
    for i in reversed(range(n_ic)):
        ic_list = tagged_struct(b'risc0_groth16.VerifyingKey.IC', [_sha(words[448 + 64 * i:512 + 64 * i]), ic_list])
    parts = [_sha(words[:64])] + [_sha(words[64 + 128 * k:192 + 128 * k]) for k in range(3)] + [ic_list]
    return tagged_struct(b'risc0_groth16.VerifyingKey', parts)


def selector_of(control_root, bn254_control_id, vk_digest):
    """calculate_selector (verifier.rs:128-144): the control id enters byte-reversed."""
    return tagged_struct(b'risc0.Groth16ReceiptVerifierParameters', [bytes(control_root), bytes(bn254_control_id)[::-1], bytes(vk_digest)])[:4]


def vk_of_words(words, n_ic=6):
    """Key words -> spec_model's vk dict."""
    w = [int.from_bytes(words[32 * i:32 * i + 32], 'big') for i in range(14 + 2 * n_ic)]
    g2 = lambda k: ((w[k], w[k + 1]), (w[k + 2], w[k + 3]))
    return dict(alpha1=(w[0], w[1]), beta2=g2(2), gamma2=g2(6), delta2=g2(10), ic=[(w[14 + 2 * i], w[15 + 2 * i]) for i in range(n_ic)])


# ---------------------------------------------------------------- routing (gateway_model.routes for this router)
def selectors_of(seals):
    return [bytes(s[:4]) if len(s) >= 4 else None for s in seals]


def routes(seals, route_selectors):
    """Route of every seal: 0 .. R - 1, NOT_FOUND or SHORT."""
    sels = [bytes(s) for s in route_selectors]
    out = np.zeros(len(seals), dtype=np.int64)
    for i, s in enumerate(selectors_of(seals)):
        out[i] = SHORT if s is None else sels.index(s) if s in sels else NOT_FOUND
    return out


def counts(route, n_routes):
    """zkv_risc0_router_last_route_counts: per route, then selector unknown, then short."""
    return [int((route == r).sum()) for r in range(n_routes)] + [int((route == NOT_FOUND).sum()), int((route == SHORT).sum())]


def selector_unknown_revert(received):
    return m.keccak256(b'SelectorUnknown(bytes4)')[:4] + bytes(received).ljust(32, b'\0')


# ---------------------------------------------------------------- per-route verifiers
def _oracle_groth16_verify(vm_type, vk, a, b, c, signals):
    """spec_model.groth16_verify's contract with the C oracle's verify_proof_with_key doing the precompile work."""
    if len(signals) + 1 != len(vk['ic']) or any(s >= m.R for s in signals):
        return False
    return ol.groth16_verify_vk(0 if vm_type == 'risc0' else 1, m.vk_to_words(vk), len(vk['ic']), m.proof_to_words(a, b, c), [m.be32(s) for s in signals])


def _with_oracle_pairing(fn, *args):
    old = m.groth16_verify
    m.groth16_verify = _oracle_groth16_verify
    try:
        return fn(*args)
    finally:
        m.groth16_verify = old


class Route:
    """One route: `verifier` is a spec_model.Risc0Verifier (built-in key) or a KeyedRisc0Verifier (caller's key, derived selector)."""

    def __init__(self, control_root, bn254_control_id, vk_words=None):
        self.control_root, self.control_id, self.words = bytes(control_root), bytes(bn254_control_id), vk_words and bytes(vk_words)
        self.keyed = vk_words is not None
        if self.keyed:
            self.vk_digest = vk_digest_of_words(self.words)
            self.selector = selector_of(control_root, bn254_control_id, self.vk_digest)
            self.verifier = sm.KeyedRisc0Verifier(vk_of_words(self.words), self.selector, self.control_root, self.control_id)
        else:
            self.vk_digest = m.risc0_vk_digest()
            self.verifier = sm.builtin_verifier(self.control_root, self.control_id)
            self.selector = self.verifier.selector
            assert self.selector == selector_of(control_root, bn254_control_id, self.vk_digest)

    def verify(self, seal, image_id, journal_digest):
        return _with_oracle_pairing(self.verifier.verify, bytes(seal), bytes(image_id), bytes(journal_digest))

    def verify_integrity(self, seal, claim_digest):
        return _with_oracle_pairing(self.verifier.verify_integrity, bytes(seal), bytes(claim_digest))


class Router:
    """Built-in routes first, then keyed routes.  ValueError where zkv_risc0_router_create returns NULL."""

    def __init__(self, builtin=(), keyed=()):
        self.routes = [Route(r, i) for r, i in builtin] + [Route(r, i, w) for w, r, i in keyed]
        sels = [r.selector for r in self.routes]
        if not self.routes or len(self.routes) > MAX_ROUTES or len(keyed) > MAX_KEYED or len(set(sels)) != len(sels):
            raise ValueError('routes')
        self.selectors = sels

    def expect(self, seals, in_a, in_b=None):
        """(status uint8[n], [received selector], route int64[n]); in_b = None: verify_integrity with claim digests in in_a."""
        route = routes(seals, self.selectors)
        st, rv = [], []
        for i, r in enumerate(route):
            if r >= 0:
                rt = self.routes[int(r)]
                s, v = rt.verify(seals[i], in_a[i], in_b[i]) if in_b is not None else rt.verify_integrity(seals[i], in_a[i])
                assert s != SELECTOR_MISMATCH
            elif r == NOT_FOUND:
                s, v = ROUTE_NOT_FOUND, bytes(seals[i][:4])
            else:
                s, v = INVALID_PROOF_DATA, None
            st.append(int(s)); rv.append(bytes(v or bytes(4)))
        return np.array(st, dtype=np.uint8), rv, route


# ---------------------------------------------------------------- the keyed group's per-slot front end (rzrouter_prep_slot)
def prep_slot(vk_valid, route, length, in_a, in_b, record):
    """(status, flags, [five signals], [ax, ay, bx_re, bx_im, by_re, by_im, cx, cy]) of one slot whose compact record is `record` (260
    bytes) and whose seal had `length` bytes; in_b = None: verify_integrity.  Signals the checks did not reach are zero, the points are
    zero unless the slot is alive; the status is the one the slot keeps unless the pairing accepts."""
    zero, nopts = [0] * 5, [0] * 8
    if length != 260:
        return INVALID_PROOF_DATA, 0, zero, nopts
    if not vk_valid or int.from_bytes(route.control_id, 'big') >= m.R:
        return VERIFICATION_FAILED, 0, zero, nopts
    claim = m.receipt_claim_ok_digest(bytes(in_a), bytes(in_b)) if in_b is not None else bytes(in_a)
    sig = route.verifier.signals(claim)
    w = [int.from_bytes(record[4 + 32 * i:36 + 32 * i], 'big') for i in range(8)]
    w[0], w[1] = m.negate_g1_words(w[0], w[1])        # groth16.rs:75-84, before the precompiles judge the coordinates
    if any(x >= m.P for x in w):
        return VERIFICATION_FAILED, 0, sig, nopts
    flags = FL_ALIVE
    a, c = (w[0], w[1]), (w[6], w[7])
    b = ((w[3], w[2]), (w[5], w[4]))                  # wire order (im, re)
    if a == (0, 0):
        flags |= FL_A_INF
    elif not m.g1_on_curve(a):
        return VERIFICATION_FAILED, 0, sig, nopts
    if c == (0, 0):
        flags |= FL_C_INF
    elif not m.g1_on_curve(c):
        return VERIFICATION_FAILED, 0, sig, nopts
    if b == ((0, 0), (0, 0)):
        flags |= FL_B_INF
    elif not m.g2_on_curve(b):
        return VERIFICATION_FAILED, 0, sig, nopts
    return VERIFICATION_FAILED, flags, sig, [w[0], w[1], w[3], w[2], w[5], w[4], w[6], w[7]]


# ---------------------------------------------------------------- fixed-seed trapdoor keys with valid seals
def params(tag):
    """(control_root, bn254_control_id) of test route `tag`: the id below R."""
    root = _sha(b'router control root ' + str(tag).encode())
    cid = (int.from_bytes(_sha(b'router control id ' + str(tag).encode()), 'big') % m.R).to_bytes(32, 'big')
    return root, cid


class Key:
    """A trapdoor key with n_ic = 6 (spec_model.trapdoor_vk, fixed seed) as a keyed route with its own control parameters."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.vk, self.td = m.trapdoor_vk(self.rng, 6)
        self.words = m.vk_to_words(self.vk)
        self.control_root, self.control_id = params(seed)
        self.route = Route(self.control_root, self.control_id, self.words)
        self.selector = self.route.selector

    def triple(self):
        return self.words, self.control_root, self.control_id

    def prove_claim(self, claim_digest):
        a, b, c = m.trapdoor_prove(self.rng, self.td, self.route.verifier.signals(bytes(claim_digest)), 'risc0')
        return self.selector + m.proof_to_words(a, b, c)

    def prove(self, image_id, journal_digest):
        """A valid 260-byte seal of this route for verify(seal, image_id, journal_digest)."""
        return self.prove_claim(m.receipt_claim_ok_digest(bytes(image_id), bytes(journal_digest)))


def off_curve_ic(words):
    """The key with IC[1].y replaced by y + 1: a point off the curve, so the key is invalid.  Its digest, hence its selector, changes too."""
    y = int.from_bytes(words[448 + 64 + 32:448 + 128], 'big')
    return words[:448 + 64 + 32] + m.be32((y + 1) % m.P) + words[448 + 128:]
