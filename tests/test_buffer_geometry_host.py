"""Where the kernels first touch the caller's bytes, without a GPU: the host builds of sha256_bytes, ShaStream, gw_ld4 / mx_ld4 and
wire_word against hashlib and plain byte arithmetic at the lengths, byte phases and alignments of tests/buffer_geometry_cases.py; the
case generators themselves against the spec model and the oracle; and the argument checks of the read-back of include/zkv_diag_prep.h,
which happen before anything touches a device.  All comparisons are exact."""
import ctypes as C
import hashlib
import os
import random
import re
import subprocess

import numpy as np
import pytest

import buffer_geometry_cases as G
import oracle_lib as ol
import plonk_model as pm
import spec_model as m

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
H = bytes.fromhex


@pytest.fixture(scope='module')
def hsg():
    src = os.path.join(HERE, 'host_sim', 'host_sim_geometry.cpp')
    lib = os.path.join(HERE, 'host_sim', 'libhost_sim_geometry.so')
    csrc = os.path.join(ROOT, 'stylus_zkvm_verifiers_amd', 'csrc')
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith('.h')]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-Wno-unknown-pragmas', '-o', lib, src])
    L = C.CDLL(lib)
    L.hsg_sha256.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.hsg_sp1_signal.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.hsg_sha_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.hsg_sha_stream.restype = C.c_size_t
    for f in (L.hsg_gw_ld4, L.hsg_mx_ld4):
        f.argtypes = [C.c_void_p, C.c_uint64]; f.restype = C.c_uint32
    L.hsg_wire_word.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return L


def _at(data, k):
    """(keep-alive array, address): `data` copied to an address that is k mod 16."""
    a = np.zeros(len(data) + 64, dtype=np.uint8)
    s = (k - a.ctypes.data) % 16
    a[s:s + len(data)] = np.frombuffer(bytes(data), dtype=np.uint8)
    return a, a.ctypes.data + s


def test_lengths_cover_every_tail_shape():
    rems = {n % 64 for n in G.LENGTHS}
    assert {0, 55, 56, 63} <= rems                                   # whole blocks, exact fit, first and last two-block tail
    assert any(n % 64 == 55 and n > 64 for n in G.LENGTHS) and any(n % 64 == 0 and n > 64 for n in G.LENGTHS)
    assert 4151 == 64 * 64 + 55 and 4151 in G.LENGTHS and 8192 in G.LENGTHS
    names = [n for n, _ in G.messages()]
    assert len(names) == len(set(names)) == len(G.LENGTHS) + 2 * len(G.PATTERN_LENGTHS)
    # a dropped `& (2^253 - 1)` shows only on a digest with one of its top three bits set: the set must hold such messages (and others)
    top = [G.top_bits_set(b) for _, b in G.messages()]
    assert sum(top) >= 8 and not all(top)
    for e in G.EDGE_LENGTHS:                                         # and at each edge length itself
        assert any(G.top_bits_set(b) for n, b in G.messages() if len(b) == e), e


def test_sha256_bytes_host_build_equals_hashlib(hsg):
    """sha256_bytes at every length and pattern, from a buffer at every byte offset 0 .. 15 (its loads are byte loads: the offset must
    not matter), and the SP1 signal formed from it as k_prep_sp1 does against hashlib's digest & (2^253 - 1)."""
    out = C.create_string_buffer(32)
    limbs = (C.c_uint32 * 8)()
    for name, msg in G.messages():
        want = hashlib.sha256(msg).digest()
        for k in range(16):
            keep, p = _at(msg, k)
            hsg.hsg_sha256(p, len(msg), out)
            assert out.raw == want, (name, k)
        keep, p = _at(msg, 1)
        hsg.hsg_sp1_signal(p, len(msg), limbs)
        got = sum(int(limbs[i]) << (32 * i) for i in range(8))
        assert got == G.expected_signal(msg) == m.sp1_hash_public_values(msg) == int.from_bytes(ol.sp1_hash_public_values(msg), 'big'), name


def test_sha256_every_length_to_two_blocks_and_a_half(hsg):
    """No length between the listed ones hides another tail shape: 0 .. 160 exhaustively."""
    out = C.create_string_buffer(32)
    rng = random.Random(5)
    for n in range(161):
        msg = rng.randbytes(n)
        keep, p = _at(msg, n % 4)
        hsg.hsg_sha256(p, n, out)
        assert out.raw == hashlib.sha256(msg).digest(), n


def _script(n, phase, rng):
    """ShaStream calls covering n bytes: `phase` single bytes first (so that every word_be / limbs_be after them starts at that byte
    phase), then a seeded mix of limbs_be, word_be and byte calls."""
    ops, left = [], n
    for _ in range(min(phase, left)):
        ops.append(0); left -= 1
    while left:
        c = rng.choice((0, 1, 1, 2)) if left >= 32 else (rng.choice((0, 1, 1)) if left >= 4 else 0)
        ops.append(c); left -= (1, 4, 32)[c]
        if c == 0 and left >= 3 and (n - left - phase) % 4 != 0:          # keep the phase: complete the group of four single bytes
            while (n - left - phase) % 4 != 0 and left:
                ops.append(0); left -= 1
    return bytes(ops)


def test_sha_stream_mixed_calls_at_every_byte_phase(hsg):
    """ShaStream (the PLONK transcripts) fed as mixed byte / word_be / limbs_be calls starting at each of the four byte phases: word_be
    takes its fast path only at phase 0 and spills into byte() otherwise; both must give hashlib's digest at every length."""
    out = C.create_string_buffer(32)
    seen = set()
    for name, msg in G.messages():
        for phase in range(4):
            ops = _script(len(msg), phase, random.Random('%s-%d' % (name, phase)))
            keep, p = _at(msg, 0)
            used = hsg.hsg_sha_stream(p, ops, len(ops), out)
            assert used == len(msg), (name, phase)
            assert out.raw == hashlib.sha256(msg).digest(), (name, phase)
            if len(msg) >= 40:
                seen.add(phase)
    assert seen == {0, 1, 2, 3}
    # words and limbs only, phase 1 .. 3: every call crosses a word of the block buffer
    for phase in range(1, 4):
        msg = random.Random(phase).randbytes(phase + 32 * 5 + 4 * 3)
        ops = bytes([0] * phase + [2, 1, 2, 2, 1, 2, 1, 2])
        keep, p = _at(msg, 0)
        assert hsg.hsg_sha_stream(p, ops, len(ops), out) == len(msg) and out.raw == hashlib.sha256(msg).digest()


def test_ld4_of_the_gather_kernels_at_every_alignment_and_tail(hsg):
    """gw_ld4 / mx_ld4 (k_gateway_gather, k_mixed_gather): up to four bytes as a little-endian word, zero padded, whichever branch the
    address selects; avail 0 .. 9."""
    rng = random.Random(11)
    data = rng.randbytes(32)
    for fn in (hsg.hsg_gw_ld4, hsg.hsg_mx_ld4):
        for k in range(8):                                            # address mod 4 = 0: the dword branch (when avail >= 4); else bytes
            keep, p = _at(data, k)
            for avail in range(10):
                take = data[:min(avail, 4)]
                assert fn(p, avail) == int.from_bytes(take + bytes(4 - len(take)), 'little'), (k, avail)


def test_wire_word_both_branches(hsg):
    """wire_word (k_wire): the value of the low four bytes (big-endian) and whether the upper 28 are zero; the dword branch on an aligned
    word and the byte branch at every alignment agree with plain byte arithmetic, a stray bit in any of the 28 upper bytes is seen."""
    rng = random.Random(13)
    out = (C.c_uint32 * 2)()
    words = [bytes(28) + rng.randbytes(4) for _ in range(4)] + [bytes(32), b'\xff' * 32]
    for i in range(28):
        words.append(bytes(i) + bytes([1 << (i % 8)]) + bytes(27 - i) + rng.randbytes(4))
    for w in words:
        want = (int.from_bytes(w[28:], 'big'), 1 if w[:28] == bytes(28) else 0)
        for k in range(8):
            keep, p = _at(w, k)
            for al in ((0, 1) if k % 4 == 0 else (0,)):
                hsg.hsg_wire_word(p, al, out)
                assert (out[0], out[1]) == want, (w.hex(), k, al)


def test_forged_plonk_proofs_verify_in_the_spec_model_and_damaged_ones_do_not():
    vk, vkb, h = G.plonk_key()
    cases = G.plonk_cases()
    assert [len(c[2]) for c in cases[:len(G.LENGTHS)]] == list(G.LENGTHS)
    for name, vkey, pv, proof, bad in cases:
        assert pm.sp1_plonk_verify_proof(vk, h, vkey, pv, proof)[0] == 0, name
        assert ol.sp1_plonk_verify_proof(vkb, h, vkey, pv, proof)[0] == 0, name
        if bad is not None:
            assert len(bad) == len(pv) and bad != pv
            assert ol.sp1_plonk_verify_proof(vkb, h, vkey, bad, proof)[0] == 1, name
    for name, vkey, pv, proof, bad in cases[::5]:                     # the (slower) spec model on a sample of the damaged ones
        if bad is not None:
            assert pm.sp1_plonk_verify_proof(vk, h, vkey, bad, proof)[0] == 1, name


def test_wire_blobs_decode_in_the_oracle_to_the_expected_records(real_proofs):
    s, r = real_proofs['sp1'], real_proofs['risc0']
    msgs = dict(G.messages())
    good = [ol.sp1_encode_call(H(s['vkey']), H(s['public_values']), H(s['proof']))]
    good += [ol.sp1_encode_call(H(s['vkey']), msgs[n], H(s['proof'])) for n in ('rand55', 'rand56', 'rand64', 'rand1')]
    recs = G.wire_blob(good)
    assert [len(b) % 4 for b, _, ok in recs if ok] == [0] * len(good)
    assert sorted(len(b) for b, _, ok in recs if not ok) == [5, 6, 7, 37, 133]
    for b, at, ok in recs:
        rev, ret, st = ol.sp1_eth_call(b)
        if ok:
            assert st == (0 if b is good[0] else 1), at               # the real proof accepts wherever it starts; other public values fail at the pairing
        else:
            assert rev and st == 6                                    # ZKV_STATUS_BAD_CALLDATA: the router cannot decode it
    orc = ol.Risc0Oracle(); orc.initialize(H(r['control_root']), H(r['bn254_control_id']))
    cd = ol.risc0_encode_call(H(r['seal']), H(r['image_id']), H(r['journal_digest']))
    for b, at, ok in G.wire_blob([cd] * 4):
        assert orc.eth_call(b)[2] == (0 if ok else 6)


def test_ragged_order_pins_the_edges():
    out = G.ragged_order(G.messages())
    assert len(out) >= 67 and {n for n, _ in out} == {n for n, _ in G.messages()}
    assert [len(out[i][1]) for i in (0, 63, 64, -1)] == list(G.EDGE_LENGTHS)


def test_prep_reader_header_declares_exactly_its_symbol():
    """include/zkv_diag_prep.h is a companion of zkv.h: its entry point is bound by diag_prep.SYMBOLS, not _lib.SYMBOLS"""
    from stylus_zkvm_verifiers_amd import _lib, diag_prep
    hdr = open(os.path.join(ROOT, 'include', 'zkv_diag_prep.h')).read()
    declared = set(re.findall(r'\b(zkv_\w+)\s*\(', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)))
    assert declared == set(diag_prep.SYMBOLS) == {'zkv_diag_prep_signals'}
    assert '#include "zkv.h"' in hdr and '#define ZKV_DIAG_PREP_SIGNALS %d' % diag_prep.SIGNALS in hdr
    zkv_h = open(os.path.join(ROOT, 'include', 'zkv.h')).read()
    for s in declared:
        assert s not in zkv_h and s not in _lib.SYMBOLS, s
    assert hasattr(diag_prep.lib(), 'zkv_diag_prep_signals')


def test_prep_reader_argument_checks(real_proofs):
    """Checked on the host before anything is launched or copied: NULL context or buffer, n = 0, a context kind without the signal rows,
    a sharded context, a context with the aggregate check on.  Acceptable arguments then meet the device check: ZKV_ERR_NO_DEVICE on a
    machine without a GPU, and (with one) ZKV_ERR_INVALID_ARG because no chunk has run on the context yet."""
    import stylus_zkvm_verifiers_amd as z
    from stylus_zkvm_verifiers_amd import _lib, diag_prep
    L = diag_prep.lib()
    r = real_proofs['risc0']
    sig = np.zeros(4 * diag_prep.SIGNALS * 8, dtype=np.uint32); fl = np.zeros(4, dtype=np.uint32)
    ps, pf = sig.ctypes.data, fl.ctypes.data
    made = []
    try:
        sp = z.Sp1Verifier(0); made.append(sp)
        v = z.RiscZeroVerifier(0); made.append(v); v.initialize(H(r['control_root']), H(r['bn254_control_id']))
        bad = _lib.ERR_INVALID_ARG
        assert L.zkv_diag_prep_signals(None, 1, ps, pf) == bad
        for ctx in (sp, v):
            assert L.zkv_diag_prep_signals(ctx._h, 1, None, pf) == bad
            assert L.zkv_diag_prep_signals(ctx._h, 1, ps, None) == bad
            assert L.zkv_diag_prep_signals(ctx._h, 0, ps, pf) == bad
        mx = z.MixedVerifier(H(r['control_root']), H(r['bn254_control_id']), 0); made.append(mx)
        pc = z.Bn254Precompiles(); made.append(pc)
        gw = z.Sp1Gateway(True, []); made.append(gw)
        for other in (mx, pc, gw):                                        # no PREP rows of their own
            assert L.zkv_diag_prep_signals(other._h, 1, ps, pf) == bad
        mk = lambda: (lambda x: (x.initialize(H(r['control_root']), H(r['bn254_control_id'])), x)[1])(z.RiscZeroVerifier(0))
        sh = z.shard([mk(), mk()]); made.append(sh)
        assert L.zkv_diag_prep_signals(sh._h, 1, ps, pf) == bad
        sp.set_aggregate_check(True)
        assert L.zkv_diag_prep_signals(sp._h, 1, ps, pf) == bad
        sp.set_aggregate_check(False)
        want = bad if z.device_count() else _lib.ERR_NO_DEVICE             # with a device: nothing has run on these contexts, n is beyond it
        for ctx in (sp, v):
            assert L.zkv_diag_prep_signals(ctx._h, 1, ps, pf) == want
        assert (sig == 0).all() and (fl == 0).all()                       # nothing was written
    finally:
        for x in made:
            x.close()
