"""Model of eth_call batches on the SP1 gateway (include/zkv_sp1_gateway_wire.h) in pure Python: a canonical encoder and a strict decoder
for both calldata forms, and the composition decode -> route (tests/gateway_model.py) -> the route's oracle (oracle_lib's SP1 Groth16 and
PLONK verifiers) -> return / revert data.  PARITY UNPINNED: the reference holds no gateway, no PLONK code and no router; where the model
overlaps the oracle (form U calls that carry the Groth16 selector) tests/test_sp1_gateway_wire_host.py ties the two together."""
import numpy as np

import gateway_model as gm
import oracle_lib as ol

FORM_U, FORM_B = 0, 1
SIGNATURES = {FORM_U: b'verifyProof(bytes32,uint8[],uint8[])', FORM_B: b'verifyProof(bytes32,bytes,bytes)'}
STATUS_OK, STATUS_BAD_CALLDATA, STATUS_ROUTE_NOT_FOUND = 0, 6, 8
BAD = -3                            # column of a request that is not a canonical call, beside gateway_model's SHORT and NOT_FOUND


def selector_of(signature):
    return ol.keccak256(bytes(signature))[:4]


def selector(form):
    return selector_of(SIGNATURES[form])


def _word(v):
    return int(v).to_bytes(32, 'big')


def pad32(n):
    return -(-n // 32) * 32


def _body(form, b):
    if form == FORM_U:
        return b''.join(_word(x) for x in b)
    return bytes(b) + bytes(pad32(len(b)) - len(b))


def encode(form, vkey, pv, proof):
    """Canonical calldata of verifyProof(vkey, pv, proof)."""
    assert len(vkey) == 32
    first = _word(len(pv)) + _body(form, pv)
    return selector(form) + bytes(vkey) + _word(0x60) + _word(0x60 + len(first)) + first + _word(len(proof)) + _body(form, proof)


def parse_header(cd):
    """Strict header rules: None, or (form, pv_at, pv_len, proof_at, proof_len) with both bodies inside the call and not a byte
    missing or left over.  Python integers: nothing wraps."""
    cd = bytes(cd)
    if len(cd) < 4:
        return None
    form = {selector(FORM_U): FORM_U, selector(FORM_B): FORM_B}.get(cd[:4])
    if form is None:
        return None
    words = lambda at: int.from_bytes(cd[at:at + 32], 'big') if at + 32 <= len(cd) else None
    span = (lambda n: 32 * n) if form == FORM_U else pad32
    o1, o2, n1 = words(36), words(68), words(100)
    if None in (o1, o2, n1) or o1 != 0x60 or n1 >= 1 << 32 or o2 != 0x80 + span(n1):
        return None
    second = 4 + o2
    n2 = words(second)
    if n2 is None or n2 >= 1 << 32 or len(cd) != second + 32 + span(n2):
        return None
    return form, 132, n1, second + 32, n2


def decode(cd):
    """None, or (form, vkey, public values, proof) of a canonical call: the header rules, every uint8[] element at most 255, every
    padding byte zero."""
    h = parse_header(cd)
    if h is None:
        return None
    form, pv_at, pv_len, proof_at, proof_len = h
    out = []
    for at, n in ((pv_at, pv_len), (proof_at, proof_len)):
        if form == FORM_U:
            body = cd[at:at + 32 * n]
            if any(body[32 * k:32 * k + 31] != bytes(31) for k in range(n)):
                return None
            out.append(bytes(body[31::32]))
        else:
            if cd[at + n:at + pad32(n)] != bytes(pad32(n) - n):
                return None
            out.append(bytes(cd[at:at + n]))
    return form, bytes(cd[4:36]), out[0], out[1]


class Gateway:
    """groth16: route 0 is the SP1 Groth16 verifier; plonk: [(vk bytes, verifier hash)], one route each, in order."""

    def __init__(self, groth16, plonk):
        self.groth16, self.plonk = bool(groth16), [(bytes(vk), bytes(vh)) for vk, vh in plonk]
        h = ol._buf(32); ol.lib().zkvo_sp1_verifier_hash(h)
        self.selectors = ([h.raw[:4]] if groth16 else []) + [vh[:4] for _, vh in self.plonk]

    def verify(self, vkey, pv, proof):
        """(status, received selector, column) of decoded arguments: the rules of include/zkv_sp1_gateway.h."""
        off = np.array([0, len(proof)], dtype=np.uint64)
        col = int(gm.routes(np.frombuffer(bytes(proof) + b'\0', np.uint8), off, self.selectors)[0])
        if col == gm.SHORT:
            return gm.STATUS_INVALID_PROOF_DATA, bytes(4), col
        if col == gm.NOT_FOUND:
            return gm.STATUS_ROUTE_NOT_FOUND, bytes(proof[:4]), col
        if self.groth16 and col == 0:
            st, rv = ol.sp1_verify_proof(vkey, pv, proof)
        else:
            vk, vh = self.plonk[col - int(self.groth16)]
            st, rv = ol.sp1_plonk_verify_proof(vk, vh, vkey, pv, proof)
        return st, bytes(rv or bytes(4)), col

    def returndata(self, status, recv):
        """(reverted, return / revert data) of one status."""
        if status == STATUS_OK:
            return False, b''
        if status == STATUS_BAD_CALLDATA:
            return True, b''
        if status == STATUS_ROUTE_NOT_FOUND:
            return True, selector_of(b'RouteNotFound(bytes4)') + bytes(recv) + bytes(28)
        return True, ol.status_abi_encode(1, status, bytes(recv), self.selectors[0])

    def eth_call(self, cd):
        """(reverted, return / revert data, status, received selector, column) of one call."""
        d = decode(cd)
        if d is None:
            st, rv, col = STATUS_BAD_CALLDATA, bytes(4), BAD
        else:
            st, rv, col = self.verify(d[1], d[2], d[3])
        rev, data = self.returndata(st, rv)
        return rev, data, st, rv, col

    def counts(self, cols):
        """zkv_sp1_gateway_last_call_counts: per route, not found, short, bad calldata."""
        cols = np.asarray(cols, dtype=np.int64)
        return gm.counts(cols, len(self.selectors)) + [int((cols == BAD).sum())]
