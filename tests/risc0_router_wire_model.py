"""Model of eth_call batches on the RISC Zero router (include/zkv_risc0_router_wire.h) in pure Python: a canonical encoder and a strict
decoder for the four call shapes (two calldata forms times verify / verifyIntegrity), and the composition decode -> route
(tests/risc0_router_model.py) -> the route's verifier -> return / revert data.  PARITY UNPINNED: the reference holds no router; form U
calls are the single RISC Zero verifier's calldata (tests/test_risc0_router_wire_host.py ties the encodings together)."""
import functools

import numpy as np

import oracle_lib as ol
import risc0_router_model as rm
import spec_model as m

FORM_U, FORM_B = 0, 1
VERIFY, INTEGRITY = 0, 1
# by call kind = 2 * form + method
SIGNATURES = {0: b'verify(uint8[],bytes32,bytes32)', 1: b'verifyIntegrity(uint8[],bytes32)',
              2: b'verify(bytes,bytes32,bytes32)', 3: b'verifyIntegrity((bytes,bytes32))'}
STATUS_OK, STATUS_BAD_CALLDATA, STATUS_ROUTE_NOT_FOUND = 0, 6, 8
BAD = -3                            # column of a request that is not a canonical call, beside risc0_router_model's SHORT and NOT_FOUND
KIND_BAD = 255


@functools.lru_cache(maxsize=None)
def selector_of(signature):
    return m.keccak256(bytes(signature))[:4]


def selector(form, method):
    return selector_of(SIGNATURES[2 * form + method])


def _word(v):
    return int(v).to_bytes(32, 'big')


def pad32(n):
    return -(-n // 32) * 32


def _body(form, b):
    if form == FORM_U:
        return b''.join(_word(x) for x in b)
    return bytes(b) + bytes(pad32(len(b)) - len(b))


def encode(form, method, seal, in_a, in_b=None):
    """Canonical calldata of verify(seal, in_a, in_b) or verifyIntegrity(seal, in_a) (form B: of the Receipt tuple (seal, in_a))."""
    assert len(in_a) == 32 and (method == INTEGRITY or len(in_b) == 32)
    tail = _word(len(seal)) + _body(form, seal)
    if method == VERIFY:
        return selector(form, method) + _word(0x60) + bytes(in_a) + bytes(in_b) + tail
    if form == FORM_U:
        return selector(form, method) + _word(0x40) + bytes(in_a) + tail
    return selector(form, method) + _word(0x20) + _word(0x40) + bytes(in_a) + tail


def parse_header(cd):
    """Strict header rules: None, or (form, method, a_at, seal_at, seal_len) with the body inside the call and not a byte missing or
    left over.  Python integers: nothing wraps."""
    cd = bytes(cd)
    if len(cd) < 4:
        return None
    kind = {selector(k >> 1, k & 1): k for k in range(4)}.get(cd[:4])
    if kind is None:
        return None
    form, method = kind >> 1, kind & 1
    word = lambda at: int.from_bytes(cd[at:at + 32], 'big') if at + 32 <= len(cd) else None
    heads = {0: [0x60], 1: [0x40], 2: [0x60], 3: [0x20, 0x40]}[kind]
    l_at = 68 if kind == 1 else 100
    n = word(l_at)
    if n is None or [word(4 + 32 * k) for k in range(len(heads))] != heads or n >= 1 << 32:
        return None
    if len(cd) != l_at + 32 + (32 * n if form == FORM_U else pad32(n)):
        return None
    return form, method, 68 if kind == 3 else 36, l_at + 32, n


def decode(cd):
    """None, or (form, method, seal, in_a, in_b or None) of a canonical call: the header rules, every uint8[] element at most 255, every
    padding byte zero."""
    h = parse_header(cd)
    if h is None:
        return None
    form, method, a_at, at, n = h
    if form == FORM_U:
        body = cd[at:at + 32 * n]
        if any(body[32 * k:32 * k + 31] != bytes(31) for k in range(n)):
            return None
        seal = bytes(body[31::32])
    else:
        if cd[at + n:at + pad32(n)] != bytes(pad32(n) - n):
            return None
        seal = bytes(cd[at:at + n])
    return form, method, seal, bytes(cd[a_at:a_at + 32]), bytes(cd[a_at + 32:a_at + 64]) if method == VERIFY else None


class WireRouter:
    """router: a risc0_router_model.Router."""

    def __init__(self, router):
        self.router = router
        self.selectors = router.selectors

    def verify(self, method, seal, in_a, in_b):
        """(status, received selector, column) of decoded arguments with a method byte: the rules of include/zkv_risc0_router.h, and
        BAD_CALLDATA for a method byte that is neither."""
        if method not in (VERIFY, INTEGRITY):
            return STATUS_BAD_CALLDATA, bytes(4), BAD
        st, rv, route = self.router.expect([bytes(seal)], [bytes(in_a)], [bytes(in_b)] if method == VERIFY else None)
        return int(st[0]), rv[0], int(route[0])

    def verify_batch(self, methods, seals, in_a, in_b):
        """(status uint8[n], [received selector], [column]) of zkv_risc0_router_verify_call_batch."""
        rows = [self.verify(int(t), s, a, b) for t, s, a, b in zip(methods, seals, in_a, in_b)]
        return np.array([r[0] for r in rows], dtype=np.uint8), [r[1] for r in rows], [r[2] for r in rows]

    def returndata(self, status, recv, kind):
        """(reverted, return / revert data) of one status: `true` for a form U success, nothing for a form B success."""
        if status == STATUS_OK:
            return False, _word(1) if kind < 2 else b''
        if status == STATUS_BAD_CALLDATA:
            return True, b''
        if status == STATUS_ROUTE_NOT_FOUND:
            return True, rm.selector_unknown_revert(recv)
        return True, ol.status_abi_encode(0, status, bytes(recv), self.selectors[0])

    def eth_call(self, cd):
        """(reverted, return / revert data, status, received selector, column, call kind) of one call."""
        d = decode(cd)
        if d is None:
            st, rv, col, kind = STATUS_BAD_CALLDATA, bytes(4), BAD, KIND_BAD
        else:
            st, rv, col = self.verify(d[1], d[2], d[3], d[4])
            kind = 2 * d[0] + d[1]
        rev, data = self.returndata(st, rv, kind)
        return rev, data, st, rv, col, kind

    def counts(self, cols):
        """zkv_risc0_router_last_call_counts: per route, selector unknown, short, bad calldata."""
        cols = np.asarray(cols, dtype=np.int64)
        return rm.counts(cols, len(self.selectors)) + [int((cols == BAD).sum())]
