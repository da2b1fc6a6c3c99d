"""Routing model of the SP1 gateway (include/zkv_sp1_gateway.h) in numpy: which route every proof of a ragged batch goes to, the
stable partition the device builds, and the per-column counts of zkv_sp1_gateway_last_route_counts.  Parity unpinned: the reference
holds no gateway; the rule is SP1VerifierGateway's (the first 4 bytes of the proof select the verifier)."""
import numpy as np

SHORT, NOT_FOUND = -1, -2          # route codes besides 0 .. R - 1
STATUS_INVALID_PROOF_DATA, STATUS_ROUTE_NOT_FOUND = 4, 8


def selectors_of(blob, off):
    """Big-endian 4-byte selector of every proof (0 where the proof is shorter than 4 bytes) and the proof lengths."""
    blob = np.asarray(blob, dtype=np.uint8)
    off = np.asarray(off, dtype=np.int64)
    lens = off[1:] - off[:-1]
    sel = np.zeros(len(lens), dtype=np.uint32)
    ok = lens >= 4
    start = off[:-1][ok]
    for k in range(4):
        sel[ok] |= blob[start + k].astype(np.uint32) << np.uint32(8 * (3 - k))
    return sel, lens


def routes(blob, off, route_selectors):
    """Route of every proof: 0 .. R - 1, NOT_FOUND or SHORT."""
    sel, lens = selectors_of(blob, off)
    out = np.full(len(lens), NOT_FOUND, dtype=np.int64)
    for r, s in enumerate(route_selectors):
        out[(sel == int.from_bytes(bytes(s), 'big')) & (out == NOT_FOUND)] = r
    out[lens < 4] = SHORT
    return out


def partition(route, n_routes):
    """Per route, the caller indices of its proofs in the order the device's records hold them (stable)."""
    return [np.nonzero(route == r)[0] for r in range(n_routes)]


def counts(route, n_routes):
    """zkv_sp1_gateway_last_route_counts: per route, then not found, then short."""
    return [int((route == r).sum()) for r in range(n_routes)] + [int((route == NOT_FOUND).sum()), int((route == SHORT).sum())]


def expected(route, blob, off, per_route):
    """Statuses and received selectors of the gateway, given per_route[r] = (status uint8[n_r], recv uint8[n_r, 4]) of route r's own
    verifier on its proofs in partition order."""
    n = len(route)
    st = np.zeros(n, dtype=np.uint8)
    rv = np.zeros((n, 4), dtype=np.uint8)
    sel, _ = selectors_of(blob, off)
    nf = route == NOT_FOUND
    st[nf] = STATUS_ROUTE_NOT_FOUND
    rv[nf] = np.stack([(sel[nf] >> np.uint32(24 - 8 * k)) & 0xFF for k in range(4)], axis=1).astype(np.uint8) if nf.any() else rv[nf]
    st[route == SHORT] = STATUS_INVALID_PROOF_DATA
    for r, idx in enumerate(partition(route, len(per_route))):
        s, v = per_route[r]
        st[idx] = s
        rv[idx] = np.asarray(v, dtype=np.uint8).reshape(-1, 4)
    return st, rv
