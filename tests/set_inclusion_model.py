"""Model of the RISC Zero set-inclusion rules of include/zkv_risc0_set_inclusion.h, on top of spec_model: the per-claim verdict is
literally V.verify(S, ID, sha256(ID || root_i)), memoised by (seal, root) so that few CPU pairings run.  PARITY UNPINNED: this file, the
host build of csrc/zkv_setincl.h and the device agree with each other, not with a reference."""
import random

import spec_model as m

MAX_DEPTH = 64
STORED = 0xFFFFFFFF
MAX_ROOTS = 4096
SET_TAG = b'risc0.SetInclusionReceiptVerifierParameters'


def leaf(claim_digest):
    return m.keccak256(b'LEAF_TAG' + claim_digest)


def node(a, b):
    return m.keccak256(min(a, b) + max(a, b))          # bytes compare as big-endian integers


def walk(claim_digest, path):
    cur = leaf(claim_digest)
    for s in path:
        cur = node(cur, s)
    return cur


def root_journal(set_id, root):
    return m.sha256(set_id + root)


def set_selector(set_id):
    return m.tagged_struct(m.sha256(SET_TAG), [set_id])[:4]


def tree_paths(leaves):
    """Every leaf's path in the tree the set builder forms: pairs are hashed level by level, an odd node moves up unpaired, so
    non-power-of-two trees give paths of mixed depth.  Returns (root, [path per leaf])."""
    paths = [[] for _ in leaves]
    level = [(lf, [i]) for i, lf in enumerate(leaves)]
    while len(level) > 1:
        nxt = []
        for k in range(0, len(level) - 1, 2):
            (a, ia), (b, ib) = level[k], level[k + 1]
            for i in ia: paths[i].append(b)
            for i in ib: paths[i].append(a)
            nxt.append((node(a, b), ia + ib))
        if len(level) % 2:
            nxt.append(level[-1])
        level = nxt
    return level[0][0], paths


class KeyedRisc0Verifier(m.Risc0Verifier):
    """`RiscZeroVerifier` with a caller-supplied key and selector (the keyed creator): the same checks in the same order."""
    def __init__(self, vk, selector, control_root, bn254_control_id):
        super().__init__()
        self.initialize(control_root, bn254_control_id)
        self.vk, self.selector = vk, bytes(selector)

    def _verify_integrity_internal(self, seal, claim_digest):
        if len(seal) < 4:
            return m.INVALID_PROOF_DATA, None
        recv = bytes(seal[:4])
        if recv != self.selector:
            return m.SELECTOR_MISMATCH, recv
        body = seal[4:]
        if len(body) != 256:
            return m.INVALID_PROOF_DATA, None
        w = [int.from_bytes(body[32 * i:32 * i + 32], 'big') for i in range(8)]
        ok = m.groth16_verify('risc0', self.vk, (w[0], w[1]), ((w[2], w[3]), (w[4], w[5])), (w[6], w[7]), self.signals(claim_digest))
        return (m.OK if ok else m.VERIFICATION_FAILED), None


def builtin_verifier(control_root, bn254_control_id):
    v = m.Risc0Verifier()
    v.initialize(control_root, bn254_control_id)
    return v


class SetVerifier:
    def __init__(self, inner, set_id):
        self.inner, self.set_id = inner, bytes(set_id)
        self.selector = set_selector(self.set_id)
        self.roots = set()
        self.memo = {}
        self.pairings = 0                           # inner verifications actually computed (the memo's misses)

    def _inner(self, seal, root):
        key = (bytes(seal), bytes(root))
        if key not in self.memo:
            self.pairings += 1
            self.memo[key] = self.inner.verify(bytes(seal), self.set_id, root_journal(self.set_id, root))
        return self.memo[key]

    def verify_claim_digest(self, claim_digest, path, root_idx, root_seals):
        """(status, received selector or None) of one claim."""
        if len(path) > MAX_DEPTH:
            return m.INVALID_PROOF_DATA, None
        if root_idx != STORED and root_idx >= len(root_seals):
            return m.INVALID_PROOF_DATA, None
        root = walk(claim_digest, path)
        if root_idx == STORED:
            return (m.OK if root in self.roots else m.VERIFICATION_FAILED), None
        return self._inner(root_seals[root_idx], root)

    def verify(self, image_id, journal_digest, path, root_idx, root_seals):
        return self.verify_claim_digest(m.receipt_claim_ok_digest(image_id, journal_digest), path, root_idx, root_seals)

    def submit_root(self, root, seal):
        st = self._inner(seal, root)
        if st[0] == m.OK:
            if root not in self.roots and len(self.roots) >= MAX_ROOTS:
                raise ValueError('more than %d roots' % MAX_ROOTS)
            self.roots.add(bytes(root))
        return st

    # ---- the on-chain form
    def encode_seal(self, path, root_seal):
        return self.selector + abi_encode_seal(path, root_seal)

    def decode_seal(self, seal):
        """(status, received selector, path, root seal)"""
        if len(seal) < 4:
            return m.INVALID_PROOF_DATA, None, None, None
        if seal[:4] != self.selector:
            return m.SELECTOR_MISMATCH, bytes(seal[:4]), None, None
        d = abi_decode_seal(seal[4:])
        if d is None:
            return m.INVALID_PROOF_DATA, None, None, None
        return m.OK, None, d[0], d[1]

    def verify_seal(self, seal, image_id, journal_digest):
        st, recv, path, root_seal = self.decode_seal(seal)
        if st != m.OK:
            return st, recv
        if not root_seal:
            return self.verify(image_id, journal_digest, path, STORED, [])
        return self.verify(image_id, journal_digest, path, 0, [root_seal])


def abi_encode_seal(path, root_seal):
    """abi.encode(Seal{bytes32[] path; bytes rootSeal})"""
    k = len(path)
    pad = -len(root_seal) % 32
    return (m.be32(0x20) + m.be32(0x40) + m.be32(0x60 + 32 * k) + m.be32(k) + b''.join(path) + m.be32(len(root_seal)) + bytes(root_seal) + bytes(pad))


def abi_decode_seal(body):
    """(path, root seal) of a canonical encoding, else None: decoding and encoding again must give the same bytes."""
    if len(body) < 160 or len(body) % 32:
        return None
    word = lambda at: int.from_bytes(body[at:at + 32], 'big')
    if word(0) != 0x20 or word(32) != 0x40:
        return None
    k = word(96)
    if k > (len(body) - 160) // 32 or word(64) != 0x60 + 32 * k:
        return None
    path = [bytes(body[128 + 32 * i:160 + 32 * i]) for i in range(k)]
    at = 128 + 32 * k
    ln = word(at)
    if ln > len(body):
        return None
    root_seal = bytes(body[at + 32:at + 32 + ln])
    if abi_encode_seal(path, root_seal) != bytes(body):
        return None
    return path, root_seal


def rng(seed):
    return random.Random(seed)
