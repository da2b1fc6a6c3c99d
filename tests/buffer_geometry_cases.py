"""TEST TOOLING -- where the kernels first touch the caller's bytes: public-values lengths around the SHA-256 block edges, base offsets
of byte-typed buffers, SP1 PLONK proofs forged to ACCEPT at every length, and calldata blobs whose records start off alignment.

Nothing here needs a GPU.  Everything is drawn from fixed seeds; the PLONK proofs come from the project's own spec model through the
trapdoor prover (plonk_trapdoor_keys.forge), as the other PLONK fixtures do (parity unpinned: the reference holds no PLONK code)."""
import functools
import hashlib
import json
import os
import random

import plonk_model as pm
import plonk_trapdoor_keys as T
import spec_model as m

HERE = os.path.dirname(os.path.abspath(__file__))

# The tail of sha256_bytes has three shapes: rem + 9 <= 64 (one block), rem + 9 > 64 (two blocks: rem = 56 .. 63), rem = 0 (a whole
# number of blocks, the tail block is padding only).  55 is the exact fit, 56 the first two-block tail, 63 the last, 64 / 128 / 8192 whole
# blocks; 119 / 120 / 121 and 183 / 184 repeat the edge after one and two full blocks; 4151 = 64 * 64 + 55 is the exact fit after a long loop.
LENGTHS = (0, 1, 31, 32, 33, 55, 56, 57, 63, 64, 65, 96, 119, 120, 121, 127, 128, 183, 184, 200, 4151, 8192)
PATTERN_LENGTHS = (55, 56, 64)                      # additionally all-0x00 and all-0xFF
EDGE_LENGTHS = (55, 56, 63, 64)                     # the lengths a ragged batch carries at index 0, 63, 64 and last
OFFSETS_BYTE = (0, 1, 2, 3)                         # base offsets of every byte-typed buffer
OFFSETS_WIDE = (4, 8, 12)                           # and where a kernel issues 8- or 16-byte loads from it
SENTINEL = 0xA5                                     # what output tensors hold outside [k, k + n)
MASK253 = (1 << 253) - 1


def messages():
    """[(name, bytes)]: seeded random bytes at every length of LENGTHS, then all-0x00 and all-0xFF at PATTERN_LENGTHS."""
    out = []
    for n in LENGTHS:
        out.append(('rand%d' % n, random.Random('buffer-geometry-pv-%d' % n).randbytes(n)))
    for n in PATTERN_LENGTHS:
        out.append(('zero%d' % n, bytes(n)))
        out.append(('ones%d' % n, b'\xff' * n))
    return out


def expected_signal(pv):
    """What the SP1 PREP kernels must derive from the public values: sha256(pv) & (2^253 - 1), from hashlib."""
    return int.from_bytes(hashlib.sha256(pv).digest(), 'big') & MASK253


def top_bits_set(pv):
    """Whether the mask changes the digest (only such a message can show a dropped mask)."""
    return hashlib.sha256(pv).digest()[0] >> 5 != 0


def ragged_order(msgs, edge=EDGE_LENGTHS, min_len=66):
    """The messages arranged as one ragged batch of at least min_len proofs with the edge lengths at index 0, 63, 64 and last (the first
    and last lanes of a wavefront, the first lane of the next, the end of the batch).  Returns a list of (name, bytes)."""
    by_len = {len(b): (n, b) for n, b in msgs if n.startswith('rand')}
    pins = [by_len[e] for e in edge]
    rest = list(msgs)
    out = list(rest)
    k = 0
    while len(out) < min_len + 1:                  # pad with the same messages again
        out.append(rest[k % len(rest)]); k += 1
    out[0] = pins[0]; out[63] = pins[1]; out[64] = pins[2]; out[-1] = pins[3]
    present = {n for n, _ in out}
    for item in msgs:                               # a pinned slot may have displaced the only copy of a message: append it before the last
        if item[0] not in present:
            out.insert(len(out) - 1, item); present.add(item[0])
    assert (len(out[0][1]), len(out[63][1]), len(out[64][1]), len(out[-1][1])) == tuple(edge)
    assert {n for n, _ in msgs} <= {n for n, _ in out}
    return out


def offset_tensor(torch, data, k, slack=64, fill=SENTINEL):
    """A uint8 device tensor holding `data` (bytes or a uint8 numpy array) from byte k on, `fill` elsewhere.  Returns (tensor, pointer):
    the pointer is data_ptr() + k, and the caller keeps the tensor alive for as long as the pointer is in use."""
    import numpy as np
    raw = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    host = np.full(k + raw.size + slack, fill, dtype=np.uint8)
    host[k:k + raw.size] = raw
    t = torch.from_numpy(host).to(torch.device('cuda', 0))
    assert t.data_ptr() % 256 == 0, 'fresh allocations are 256-byte aligned: the offsets below are the alignment under test'
    return t, t.data_ptr() + k


def outside_is_sentinel(t, k, n, fill=SENTINEL):
    """Bytes of the output tensor t outside [k, k + n) kept their sentinel."""
    h = t.cpu().numpy()
    return bool((h[:k] == fill).all() and (h[k + n:] == fill).all())


# ---------------------------------------------------------------- SP1 PLONK proofs that ACCEPT at every length
@functools.lru_cache(maxsize=None)
def plonk_key():
    """(trapdoor key dict, key bytes, verifier hash) of the SP1 PLONK key of these tests (two public inputs, one commitment)."""
    vk = T.make_key(T.rng_for('buffer-geometry-plonk-key'), 2, 1)
    vkb = pm.vk_bytes(vk)
    return vk, vkb, hashlib.sha256(b'buffer geometry sp1 plonk route' + vkb).digest()


def flip_byte(b, rng):
    """One byte of b changed (b not empty)."""
    i = rng.randrange(len(b))
    return b[:i] + bytes([b[i] ^ (1 << rng.randrange(8))]) + b[i + 1:]


@functools.lru_cache(maxsize=None)
def plonk_cases():
    """[(name, program vkey, public values, proof bytes (selector + 27 words), flipped public values or None)]: one forged proof per
    message of messages(); it verifies for its public values and (length > 0) not for the flipped ones."""
    vk, _, h = plonk_key()
    out = []
    for name, pv in messages():
        rng = T.rng_for('buffer-geometry-plonk-proof', name)
        vkey = rng.randrange(m.R).to_bytes(32, 'big')
        proof = h[:4] + T.forge(vk, [int.from_bytes(vkey, 'big'), expected_signal(pv) % m.R], rng)
        out.append((name, vkey, pv, proof, flip_byte(pv, rng) if pv else None))
    return out


# ---------------------------------------------------------------- calldata blobs whose records start off alignment
def real():
    with open(os.path.join(HERE, 'golden', 'real_proofs.json')) as f:
        return json.load(f)


def misaligning_records():
    """Malformed records of 5, 6, 7 and 4 + 32 k + 1 bytes (k = 1, 4): every byte string that is not canonical calldata."""
    rng = random.Random('buffer-geometry-junk')
    return [rng.randbytes(n) for n in (5, 6, 7, 4 + 32 * 1 + 1, 4 + 32 * 4 + 1)]


def wire_blob(good):
    """`good`: canonical calldata records (lengths are multiples of 4 plus 0: 4 + 32 k).  Returns the records of one blob in which
    malformed records of 5, 6, 7, 37 and 133 bytes separate them, so that well-formed records start at offsets 0, 1, 3, 2 ... mod 4;
    every residue occurs.  [(bytes, start offset mod 4, is_good)]"""
    junk = misaligning_records()
    recs, at, k = [], 0, 0
    for g in good:
        recs.append((g, at % 4, True)); at += len(g)
        j = junk[k % len(junk)]; k += 1
        recs.append((j, at % 4, False)); at += len(j)
    assert {a for _, a, ok in recs if ok} == {0, 1, 2, 3}, 'every residue mod 4 starts a well-formed record'
    return recs
