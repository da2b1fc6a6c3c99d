"""Model of eth_call batches and per-seal methods on a RISC Zero router with a set route (include/zkv_risc0_router_set_wire.h): the
composition risc0_router_wire_model.WireRouter(risc0_router_set_model.SetRouter(...)) -- the calldata layer in front of the router in
front of the set verifier, no new arithmetic -- with the route_count + 3 counts of zkv_risc0_router_last_ragged_call_counts and the
four counts of zkv_risc0_router_set_last_counts for a batch.  PARITY UNPINNED: the reference holds no router and no set verifier."""
import numpy as np

import risc0_router_model as rm
import risc0_router_set_model as rsm
import risc0_router_wire_model as wm
import spec_model as m
from wire_util import apply_ops

FORM_U, FORM_B, VERIFY, INTEGRITY, KIND_BAD = wm.FORM_U, wm.FORM_B, wm.VERIFY, wm.INTEGRITY, wm.KIND_BAD
STATUS_BAD_CALLDATA = wm.STATUS_BAD_CALLDATA
SET = rsm.SET                         # column of a seal with the set selector
BAD = -4                              # column of a request that is not a canonical call (wm.BAD is rsm.SET's number)
H = bytes.fromhex


def in_a_of(it, method):
    """The first input of a call on fixture item `it`: the image id, or (verifyIntegrity) the claim digest -- the item's own where it
    names one (a wrong digest on purpose), else that of its image id and journal digest."""
    a, b = H(it['image_id']), H(it['journal_digest'])
    if method == VERIFY:
        return a
    return H(it['claim_digest']) if it.get('claim_digest') else m.receipt_claim_ok_digest(a, b)


def calldata_of(it, form, method, ops=()):
    return apply_ops(wm.encode(form, method, H(it['seal']), in_a_of(it, method), H(it['journal_digest']) if method == VERIFY else None), ops)


def load_fixture(path):
    """tests/golden/risc0_router_set_wire_cases.json with every edited item written out and every case's name ("Uv: ...", the edits' tag in front of the item's name) and
    calldata."""
    import json
    d = json.load(open(path))
    for k, it in enumerate(d['items']):
        if 'base' in it:                                             # an edited seal: the base item's seal with the edits, its inputs unless given
            base = d['items'][it['base']]
            d['items'][k] = dict(base, **dict(it, seal=apply_ops(H(base['seal']), it['ops']).hex()))
    d['cases'] = [dict(zip(d['case_fields'], row)) for row in d['cases']]
    for c in d['cases']:
        it = d['items'][c['item']]
        c['name'] = '%s%s: %s' % ('UB'[c['form']], 'vi'[c['method']], '%s [%s]' % (c['tag'], it['name']) if c['tag'] else it['name'])
        c['calldata'] = calldata_of(it, c['form'], c['method'], c['ops'])
        assert len(c['calldata']) == c['calldata_len'], c['name']
    return d


class SetWireRouter(wm.WireRouter):
    """set_router: a risc0_router_set_model.SetRouter."""

    def __init__(self, set_router):
        super().__init__(set_router)
        self.set_router = set_router

    def verify(self, method, seal, in_a, in_b):
        st, rv, col = super().verify(method, seal, in_a, in_b)
        return st, bytes(rv), (BAD if method not in (VERIFY, INTEGRITY) else col)

    def eth_call(self, cd):
        rev, data, st, rv, col, kind = super().eth_call(cd)
        return rev, data, st, bytes(rv), (BAD if kind == KIND_BAD else col), kind

    def counts(self, cols):
        """zkv_risc0_router_last_ragged_call_counts: per Groth16 route, the set route, selector unknown, short, bad calldata."""
        cols = np.asarray(cols, dtype=np.int64)
        R = len(self.set_router.router.routes)
        return [int((cols == r).sum()) for r in range(R)] + [int((cols == c).sum()) for c in (SET, rm.NOT_FOUND, rm.SHORT, BAD)]

    def _batch(self, rows):
        cols = [r[-2] if len(r) == 6 else r[2] for r in rows]
        s = self.set_router
        return dict(rows=rows, columns=cols, counts=self.counts(cols),
                    set_counts=(sum(1 for c in cols if c == SET), len(s.root_seals), s.pairings, s.lookups))

    def eth_call_batch(self, calls):
        """One batch (one chunk) in the caller's order: rows of eth_call, the columns, `counts` and `set_counts` -- set seals, distinct
        root seals among their claims, root jobs of the grouping rule (one per group and one per straggler), stored-root lookups."""
        self.set_router.reset_counts()
        return self._batch([self.eth_call(cd) for cd in calls])

    def verify_call_batch(self, methods, seals, in_a, in_b):
        """The decoded-input call: rows of (status, received selector, column)."""
        self.set_router.reset_counts()
        return self._batch([self.verify(int(t), s, a, b) for t, s, a, b in zip(methods, seals, in_a, in_b)])
