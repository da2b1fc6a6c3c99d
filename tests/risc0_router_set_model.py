"""Model of a RISC Zero router with a set route (include/zkv_risc0_router_set.h): risc0_router_model.Router for the Groth16 routes,
set_inclusion_model.SetVerifier with THAT ROUTER as its inner verifier for the set route, and in front of both the routing rule and the
one library limit the set verifier's model does not know -- a root seal that itself begins with the set selector is not followed.  One
seal at a time, as on chain; the per-claim verdict is literally router.verify(S, ID, sha256(ID || root_i)), memoised by (S, root);
`pairings` counts the root jobs a batch needs.  PARITY UNPINNED: the reference holds no router and no set verifier."""
import numpy as np

import risc0_router_model as rm
import set_inclusion_model as sm
import spec_model as m

OK, VERIFICATION_FAILED, INVALID_PROOF_DATA, ROUTE_NOT_FOUND = rm.OK, rm.VERIFICATION_FAILED, rm.INVALID_PROOF_DATA, rm.ROUTE_NOT_FOUND
SET = -3                              # route code of a seal with the set selector, beside risc0_router_model's SHORT and NOT_FOUND


class _RouterAsVerifier:
    """The router behind IRiscZeroVerifier.verify, as the set verifier's VERIFIER sees it."""

    def __init__(self, router):
        self.router = router

    def verify(self, seal, image_id, journal_digest):
        st, rv, _ = self.router.expect([bytes(seal)], [bytes(image_id)], [bytes(journal_digest)])
        return int(st[0]), (rv[0] if any(rv[0]) else None)


class SetRouter:
    """builtin / keyed as risc0_router_model.Router; ValueError where zkv_risc0_router_create_with_set returns NULL."""

    def __init__(self, set_id, builtin=(), keyed=()):
        self.router = rm.Router(builtin, keyed)
        self.set_id = bytes(set_id)
        self.set = sm.SetVerifier(_RouterAsVerifier(self.router), self.set_id)
        self.set_selector = self.set.selector
        if len(self.router.routes) + 1 > rm.MAX_ROUTES or self.set_selector in self.router.selectors:
            raise ValueError('routes')
        self.selectors = self.router.selectors + [self.set_selector]
        self.reset_counts()

    def reset_counts(self):
        """What zkv_risc0_router_set_last_counts reports of the seals verified from here on, in this order (one chunk): the distinct root
        seals their claims carried (rep_root: each with the root of the first claim carrying it, the group's representative), the
        stragglers -- claims whose root differs from their representative's, each verified on its own -- and the stored-root lookups.
        The memo of inner verdicts stays: a verdict does not depend on the batch."""
        self.rep_root, self.stragglers, self.lookups = {}, 0, 0

    @property
    def root_seals(self):
        return set(self.rep_root)

    @property
    def pairings(self):
        """Root jobs the grouping rule runs: one per group and one per straggler (two stragglers with one root are two jobs)."""
        return len(self.rep_root) + self.stragglers

    def encode_seal(self, path, root_seal=b''):
        return self.set.encode_seal(path, root_seal)

    def submit_root(self, root, seal):
        return self.set.submit_root(bytes(root), bytes(seal))

    def route(self, seal):
        if len(seal) >= 4 and bytes(seal[:4]) == self.set_selector:
            return SET
        return int(rm.routes([seal], self.router.selectors)[0])

    def _set_seal(self, seal, claim_digest):
        d = sm.abi_decode_seal(bytes(seal[4:]))
        if d is None:
            return INVALID_PROOF_DATA, None
        path, root_seal = d
        if len(path) > sm.MAX_DEPTH or root_seal[:4] == self.set_selector:      # library limits: no hashing, no pairing
            return INVALID_PROOF_DATA, None
        root = sm.walk(claim_digest, path)           # (SetVerifier.verify_claim_digest from here on, with the root kept for the counts)
        if not root_seal:
            self.lookups += 1
            return (OK if root in self.set.roots else VERIFICATION_FAILED), None
        if self.rep_root.setdefault(root_seal, root) != root:
            self.stragglers += 1
        return self.set._inner(root_seal, root)

    def verify_integrity(self, seal, claim_digest):
        """(status, received selector (4 bytes, zero when none))"""
        seal = bytes(seal)
        if self.route(seal) == SET:
            st, rv = self._set_seal(seal, bytes(claim_digest))
        else:
            s, v, _ = self.router.expect([seal], [bytes(claim_digest)])
            st, rv = int(s[0]), v[0]
        return int(st), bytes(rv or bytes(4))

    def verify(self, seal, image_id, journal_digest):
        seal = bytes(seal)
        if self.route(seal) == SET:
            st, rv = self._set_seal(seal, m.receipt_claim_ok_digest(bytes(image_id), bytes(journal_digest)))
            return int(st), bytes(rv or bytes(4))
        s, v, _ = self.router.expect([seal], [bytes(image_id)], [bytes(journal_digest)])
        return int(s[0]), bytes(v[0] or bytes(4))

    def expect(self, seals, in_a, in_b=None):
        """(status uint8[n], [received selector], route int[n]) of a batch; in_b = None: verify_integrity.  Afterwards `pairings`,
        `root_seals` and `lookups` describe the batch (reset_counts first)."""
        st, rv, route = [], [], []
        for i, seal in enumerate(seals):
            s, v = self.verify(seal, in_a[i], in_b[i]) if in_b is not None else self.verify_integrity(seal, in_a[i])
            st.append(s); rv.append(v); route.append(self.route(seal))
        return np.array(st, dtype=np.uint8), rv, np.array(route, dtype=np.int64)

    def counts(self, route):
        """zkv_risc0_router_last_route_counts of a set-routed router: the Groth16 routes, the set route, unknown, short."""
        R = len(self.router.routes)
        return [int((route == r).sum()) for r in range(R)] + [int((route == SET).sum()), int((route == rm.NOT_FOUND).sum()), int((route == rm.SHORT).sum())]
