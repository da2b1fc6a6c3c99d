"""Model of the SP1 gateway's Groth16 routes with caller-supplied keys (include/zkv_sp1_gateway_keys.h): `sp1_verify_proof` of
oracle/spec_model.py with the verifier hash and the key as parameters (the pairing by the C oracle's verify_proof_with_key), the
per-slot front end the device runs before the pairing (csrc/zkv_gwset_prep.h), and fixed-seed trapdoor keys with valid proofs.
A route holding the reference's own key and hash is reference-pinned; PARITY UNPINNED for every other key."""
import hashlib
import random

import oracle_lib as ol
import spec_model as m

OK, VERIFICATION_FAILED, INVALID_PROOF_DATA, SELECTOR_MISMATCH = 0, 1, 4, 5
FL_ALIVE, FL_A_INF, FL_B_INF, FL_C_INF = 1, 2, 4, 8
VM_SP1 = 1                      # the C oracle's vm argument


def sp1_verify_proof(vk_words, verifier_hash, program_vkey, public_values, proof_bytes):
    """sp1/verifier.rs:58-111 with `verifier_hash` for VERIFIER_HASH and `vk_words` (n_ic = 3) for the key -> (status, received)."""
    if len(proof_bytes) < 4:
        return INVALID_PROOF_DATA, None
    recv = bytes(proof_bytes[:4])
    if recv != bytes(verifier_hash[:4]):
        return SELECTOR_MISMATCH, recv
    body = bytes(proof_bytes[4:])
    if len(body) != 256:
        return INVALID_PROOF_DATA, None
    signals = [int.from_bytes(program_vkey, 'big'), m.sp1_hash_public_values(public_values)]
    if any(s >= m.R for s in signals):
        return VERIFICATION_FAILED, None
    ok = ol.groth16_verify_vk(VM_SP1, vk_words, 3, body, [m.be32(s) for s in signals])
    return (OK if ok else VERIFICATION_FAILED), None


def prep_slot(vk_valid, length, program_vkey, public_values, record):
    """gwset_prep_slot: (status, flags, signal 0, signal 1) of one slot whose compact record is `record` (260 bytes) and whose proof had
    `length` bytes.  A signal the checks did not reach is zero; the status is the one the slot keeps unless the pairing accepts."""
    if length != 260:
        return INVALID_PROOF_DATA, 0, 0, 0
    if not vk_valid:
        return VERIFICATION_FAILED, 0, 0, 0
    s0 = int.from_bytes(program_vkey, 'big')
    if s0 >= m.R:
        return VERIFICATION_FAILED, 0, s0, 0
    s1 = int.from_bytes(hashlib.sha256(bytes(public_values)).digest(), 'big') & m.SP1_FIELD_MASK
    w = [int.from_bytes(record[4 + 32 * i:36 + 32 * i], 'big') for i in range(8)]
    if any(x >= m.P for x in w):
        return VERIFICATION_FAILED, 0, s0, s1
    flags = FL_ALIVE
    a, c = (w[0], w[1]), (w[6], w[7])
    b = ((w[3], w[2]), (w[5], w[4]))                  # wire order (im, re)
    if a == (0, 0):
        flags |= FL_A_INF
    elif not m.g1_on_curve(a):
        return VERIFICATION_FAILED, 0, s0, s1
    if c == (0, 0):
        flags |= FL_C_INF
    elif not m.g1_on_curve(c):
        return VERIFICATION_FAILED, 0, s0, s1
    if b == ((0, 0), (0, 0)):
        flags |= FL_B_INF
    elif not m.g2_on_curve(b):
        return VERIFICATION_FAILED, 0, s0, s1
    return VERIFICATION_FAILED, flags, s0, s1


def verifier_hash(tag):
    """A 32-byte verifier hash for test route `tag` (its first four bytes are the selector)."""
    return hashlib.sha256(b'keyed SP1 Groth16 route ' + str(tag).encode()).digest()


class Key:
    """A trapdoor key with n_ic = 3 (spec_model.trapdoor_vk, fixed seed) and its route's verifier hash."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.vk, self.td = m.trapdoor_vk(self.rng, 3)
        self.words = m.vk_to_words(self.vk)
        self.hash = verifier_hash(seed)
        self.selector = self.hash[:4]

    def prove(self, program_vkey, public_values):
        """A valid 260-byte proof of this route for (program_vkey, public_values)."""
        sig = [int.from_bytes(program_vkey, 'big'), m.sp1_hash_public_values(public_values)]
        a, b, c = m.trapdoor_prove(self.rng, self.td, sig, 'sp1')
        return self.selector + m.proof_to_words(a, b, c)

    def verify(self, program_vkey, public_values, proof):
        st, rv = sp1_verify_proof(self.words, self.hash, program_vkey, public_values, proof)
        return st, bytes(rv or bytes(4))


def off_curve_ic(words):
    """The key with IC[1].y replaced by y + 1: a point off the curve, so the key is invalid."""
    y = int.from_bytes(words[448 + 64 + 32:448 + 128], 'big')
    return words[:448 + 64 + 32] + m.be32((y + 1) % m.P) + words[448 + 128:]
