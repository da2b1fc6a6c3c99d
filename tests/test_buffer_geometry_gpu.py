"""Where the kernels first touch the caller's bytes, on the device: the SHA-256 of SP1 public values at every length of
tests/buffer_geometry_cases.py (read back through include/zkv_diag_prep.h on the Groth16 path, by ACCEPT on the PLONK path), the RISC
Zero claim-digest chain, device buffers at base offsets that are not multiples of four, calldata blobs whose records start off
alignment, and the real SP1 proof at the first / wave-boundary / last positions of ragged batches.  All comparisons are exact.

Every cell (path, case, alignment) that runs is recorded; the last test compares the record with the cells the generators define.

The uint32 / uint64 arguments (instance and key indices, offsets) keep their natural alignment, as the headers require."""
import ctypes as C
import hashlib
import os
import random

import numpy as np
import pytest

import buffer_geometry_cases as G
import oracle_lib as ol
import plonk_model as pm
import spec_model as m

pytestmark = pytest.mark.gpu
H = bytes.fromhex
RAN = []                                           # (path, case, alignment) of every cell that ran and passed


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


@pytest.fixture(scope='module')
def sp(zkv):
    v = zkv.Sp1Verifier(0)
    yield v
    v.close()


@pytest.fixture(scope='module')
def r0(zkv, real_proofs):
    r = real_proofs['risc0']
    v = zkv.RiscZeroVerifier(0); v.initialize(H(r['control_root']), H(r['bn254_control_id']))
    yield v
    v.close()


def _signals(handle, n):
    from stylus_zkvm_verifiers_amd import diag_prep
    return diag_prep.prep_signals(handle, n)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _sp1_batch(real_proofs):
    """The messages in ragged order (edge lengths at 0, 63, 64, last) under the real proof's seal and vkey, with the real public values
    at index 1: [(name, pv)]."""
    batch = G.ragged_order(G.messages())
    batch[1] = ('real', H(real_proofs['sp1']['public_values']))
    return batch


def _check_sp1(batch, st, sig, fl, vkey, proof, path, align=0):
    for j, (name, pv) in enumerate(batch):
        want = ol.sp1_verify_proof(vkey, pv, proof)[0]
        assert int(st[j]) == want == (0 if name == 'real' else 1), (path, name, j)
        assert fl[j] != 0, (path, name, j)                            # valid points: PREP stored the signals
        assert sig[j][0] == int.from_bytes(vkey, 'big'), (path, name, j)
        assert sig[j][1] == G.expected_signal(pv) == int.from_bytes(ol.sp1_hash_public_values(pv), 'big'), (path, name, j, len(pv))
        assert sig[j][2:] == [0, 0, 0]
        if name != 'real':
            RAN.append((path, name, align))


# ---------------------------------------------------------------- digest by read-back, SP1 Groth16
def test_sp1_digest_read_back_ragged_host_call(zkv, sp, real_proofs):
    s = real_proofs['sp1']
    vkey, proof = H(s['vkey']), H(s['proof'])
    batch = _sp1_batch(real_proofs)
    n = len(batch)
    st, _ = sp.verify_batch([vkey] * n, [pv for _, pv in batch], [proof] * n)
    sig, fl = _signals(sp._h, n)
    assert any(G.top_bits_set(pv) for _, pv in batch)                  # the `& (2^253 - 1)` is visible in this batch
    _check_sp1(batch, st, sig, fl, vkey, proof, 'sp1-host-ragged')
    # n beyond the last chunk is refused, n inside it is not
    from stylus_zkvm_verifiers_amd import _lib, diag_prep
    buf = np.zeros((n + 1) * 40, dtype=np.uint32)
    assert diag_prep.lib().zkv_diag_prep_signals(sp._h, n + 1, buf.ctypes.data, buf.ctypes.data) == _lib.ERR_INVALID_ARG
    assert diag_prep.lib().zkv_diag_prep_signals(sp._h, 1, buf.ctypes.data, buf[40:].ctypes.data) == _lib.OK


def test_sp1_digest_read_back_device_call_at_every_length_and_offset(zkv, sp, real_proofs):
    """zkv_sp1_verify_batch_dev with pv_len = every length: 66 rows at a fixed stride (odd lengths put every later row off alignment
    anyway), the public-values buffer itself at base offsets 0 .. 3; rows differ in their first byte where there is one."""
    _sp1_dev_lengths(sp, real_proofs, G.messages() + [('real', H(real_proofs['sp1']['public_values']))])


def _sp1_dev_lengths(sp, real_proofs, msgs):
    import torch
    s = real_proofs['sp1']
    vkey, proof = H(s['vkey']), H(s['proof'])
    n = 66
    d_vk = torch.from_numpy(np.tile(np.frombuffer(vkey, dtype=np.uint8), n)).cuda()
    d_p = torch.from_numpy(np.tile(np.frombuffer(proof, dtype=np.uint8), n)).cuda()
    for name, pv in msgs:
        rows = [pv if (j in (0, 63, 64, n - 1) or not pv) else bytes([(pv[0] + j) & 255]) + pv[1:] for j in range(n)]
        for k in G.OFFSETS_BYTE:
            keep, p_pv = G.offset_tensor(torch, b''.join(rows), k)
            d_st = torch.full((n,), 255, dtype=torch.uint8, device='cuda')
            sp.verify_batch_dev(n, d_vk.data_ptr(), p_pv, len(pv), d_p.data_ptr(), d_st.data_ptr(), 0, _stream())
            torch.cuda.synchronize()
            st = d_st.cpu().numpy()
            sig, fl = _signals(sp._h, n)
            for j in range(n):
                assert fl[j] != 0 and sig[j][1] == G.expected_signal(rows[j]), (name, k, j)
                assert int(st[j]) == (0 if name == 'real' and rows[j] == pv else 1), (name, k, j)
            if name != 'real':
                RAN.append(('sp1-dev', name, k))


def test_sp1_digest_read_back_wire_path(zkv, sp, real_proofs):
    """The wire decoder produces the pv_len[] records: every length as eth_call calldata in one batch, then the same records separated by
    malformed ones of 5, 6, 7, 37 and 133 bytes (later records start at 1, 2, 3 mod 4: the decoder's byte branches)."""
    s = real_proofs['sp1']
    vkey, proof = H(s['vkey']), H(s['proof'])
    batch = _sp1_batch(real_proofs)
    cds = [zkv.wire.encode_sp1_verify_proof(vkey, pv, proof) for _, pv in batch]
    assert cds[0] == ol.sp1_encode_call(vkey, batch[0][1], proof)
    rev, ret, st = zkv.wire.eth_call_batch(sp, cds)
    sig, fl = _signals(sp._h, len(batch))
    _check_sp1(batch, st, sig, fl, vkey, proof, 'sp1-wire')
    for j, cd in enumerate(cds):
        assert (bool(rev[j]), ret[j]) == ol.sp1_eth_call(cd)[:2], batch[j][0]
    # misaligning records between the well-formed ones
    recs = G.wire_blob(cds)
    rev, ret, st = zkv.wire.eth_call_batch(sp, [b for b, _, _ in recs])
    sig, fl = _signals(sp._h, len(recs))
    seen = set()
    for j, (b, at, ok) in enumerate(recs):
        o_rev, o_ret, o_st = ol.sp1_eth_call(b)
        assert (bool(rev[j]), ret[j]) == (o_rev, o_ret), (j, at, ok)
        if ok:
            name, pv = batch[j // 2]
            assert int(st[j]) == o_st == (0 if name == 'real' else 1), (name, at)
            assert fl[j] != 0 and sig[j][1] == G.expected_signal(pv), (name, at)
            seen.add(at)
            if name != 'real':
                RAN.append(('sp1-wire-misaligned', name, at))
        else:
            assert int(st[j]) == 6 and fl[j] == 0, (j, at)
    assert seen == {0, 1, 2, 3}
    assert int(st[2]) == 0 and recs[2][1] != 0                         # the real proof still ACCEPTS behind a misaligning record


def test_wire_blob_with_an_offset_base_pointer(zkv, sp, r0, real_proofs):
    """zkv_eth_call_batch_dev on a blob whose base pointer is 1, 2, 3 bytes off (and whose records are separated by malformed ones):
    statuses and received selectors equal the aligned run and the oracle; both VMs."""
    import torch
    s, r = real_proofs['sp1'], real_proofs['risc0']
    msgs = dict(G.messages())
    orc = ol.Risc0Oracle(); orc.initialize(H(r['control_root']), H(r['bn254_control_id']))
    bad_seal = H(r['seal'])[:-1] + bytes([H(r['seal'])[-1] ^ 1])
    good = {
        'sp1': [zkv.wire.encode_sp1_verify_proof(H(s['vkey']), pv, H(s['proof']))
                for pv in (H(s['public_values']), msgs['rand55'], H(s['public_values']), msgs['rand56'], H(s['public_values']), msgs['rand64'])]
               + [zkv.wire.encode_sp1_verify_proof(H(s['vkey']), H(s['public_values']), b'\x01\x02\x03\x04' + H(s['proof'])[4:])],
        'risc0': [zkv.wire.encode_risc0_verify(H(r['seal']), H(r['image_id']), H(r['journal_digest'])),
                  zkv.wire.encode_risc0_verify_integrity(H(r['seal']), H(r['claim_digest'])),
                  zkv.wire.encode_risc0_verify(bad_seal, H(r['image_id']), H(r['journal_digest'])),
                  zkv.wire.encode_risc0_verify(H(r['seal']), H(r['image_id']), H(r['journal_digest'])),
                  zkv.wire.encode_risc0_verify(b'\x00\x00\x00\x01' + H(r['seal'])[4:], H(r['image_id']), H(r['journal_digest'])),
                  zkv.wire.encode_risc0_verify_integrity(H(r['seal']), H(r['claim_digest']))]}
    for vm, ver in (('sp1', sp), ('risc0', r0)):
        recs = G.wire_blob(good[vm])
        calls = [(ol.sp1_eth_call(b) if vm == 'sp1' else orc.eth_call(b)) for b, _, _ in recs]
        want = [c[2] for c in calls]
        assert want.count(0) >= 3 and 5 in want
        expected_sel = sp.verifier_hash()[:4] if vm == 'sp1' else orc.get_selector()
        n = len(recs)
        off = np.zeros(n + 1, dtype=np.uint64); off[1:] = np.cumsum([len(b) for b, _, _ in recs])
        d_off = torch.from_numpy(off.view(np.int64)).cuda()
        base = None
        for k in G.OFFSETS_BYTE + G.OFFSETS_WIDE:                      # 4, 8, 12: the other phases of the decoder's 16-byte loads
            keep, p_cd = G.offset_tensor(torch, b''.join(b for b, _, _ in recs), k)
            for ko in (0, k % 4):                                      # outputs aligned, then moved with the blob
                t_st, p_st = G.offset_tensor(torch, bytes([255]) * n, ko)
                t_rv, p_rv = G.offset_tensor(torch, bytes([255]) * (4 * n), ko)
                zkv.wire.eth_call_batch_dev(ver, n, p_cd, d_off.data_ptr(), int(off[-1]), p_st, p_rv, _stream())
                torch.cuda.synchronize()
                st = t_st.cpu().numpy()[ko:ko + n]; rv = t_rv.cpu().numpy()[ko:ko + 4 * n]
                assert [int(x) for x in st] == want, (vm, k, ko)
                assert G.outside_is_sentinel(t_st, ko, n) and G.outside_is_sentinel(t_rv, ko, 4 * n), (vm, k, ko)
                if base is None:
                    base = rv.copy()
                assert (rv == base).all(), (vm, k, ko)
                # the return data a caller forms from (status, received selector) is the oracle's, for every verify-class call
                for j, (o_rev, o_ret, o_st) in enumerate(calls):
                    if o_st != 6:
                        assert o_rev == (o_st != 0), (vm, j)
                        enc = ol.status_abi_encode(0 if vm == 'risc0' else 1, o_st, rv[4 * j:4 * j + 4].tobytes(), expected_sel)
                        assert (enc if o_rev else b'') == (o_ret if o_rev else b''), (vm, k, ko, j)
            RAN.append(('wire-dev-' + vm, 'blob', k))


# ---------------------------------------------------------------- RISC Zero claim-digest chain by read-back
def test_risc0_claim_digest_halves_read_back(zkv, r0, real_proofs):
    """Seeded random (image_id, journal_digest) pairs through verify, and claim digests through verify_integrity, under the real seal:
    the two 128-bit halves PREP derived equal the oracle's claim digest split as the reference splits it."""
    r = real_proofs['risc0']
    seal = H(r['seal'])
    rng = random.Random('buffer-geometry-risc0')
    pairs = [(H(r['image_id']), H(r['journal_digest']))] + [(rng.randbytes(32), rng.randbytes(32)) for _ in range(129)]
    pairs += [(bytes(32), bytes(32)), (b'\xff' * 32, b'\xff' * 32)]

    def halves(d):
        rev = d[::-1]
        return int.from_bytes(rev[16:], 'big'), int.from_bytes(rev[:16], 'big')
    assert ['%064x' % x for x in halves(H(r['claim_digest']))] == r['signals'][2:4]
    st, _ = r0.verify_batch([seal] * len(pairs), [a for a, _ in pairs], [b for _, b in pairs])
    sig, fl = _signals(r0._h, len(pairs))
    for j, (a, b) in enumerate(pairs):
        d = ol.risc0_claim_digest(a, b)
        assert fl[j] != 0 and tuple(sig[j][:2]) == halves(d) and sig[j][2:] == [0, 0, 0], j
        assert int(st[j]) == (0 if j == 0 else 1)
    claims = [H(r['claim_digest'])] + [rng.randbytes(32) for _ in range(129)] + [bytes(32), b'\xff' * 32]
    st, _ = r0.verify_integrity_batch([seal] * len(claims), claims)
    sig, fl = _signals(r0._h, len(claims))
    for j, d in enumerate(claims):
        assert fl[j] != 0 and tuple(sig[j][:2]) == halves(d), j
        assert int(st[j]) == (0 if j == 0 else 1)
    RAN.append(('risc0-claim', 'pairs', 0)); RAN.append(('risc0-claim', 'integrity', 0))


# ---------------------------------------------------------------- digest by ACCEPT, SP1 PLONK
def test_plonk_accepts_at_every_length_on_every_path(zkv, real_proofs):
    import torch
    vk, vkb, h = G.plonk_key()
    cases = G.plonk_cases()
    rows = []                                                         # (name, vkey, pv, proof, want)
    for name, vkey, pv, proof, bad in cases:
        rows.append((name, vkey, pv, proof, 0))
        if bad is not None:
            rows.append((name + '-flipped', vkey, bad, proof, 1))
    for name, vkey, pv, proof, want in rows:
        assert pm.sp1_plonk_verify_proof(vk, h, vkey, pv, proof)[0] == want, name
    v = zkv.Sp1PlonkVerifier(vkb, h)
    st, _ = v.verify_batch([r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows])
    for r_, x in zip(rows, st):
        assert int(x) == r_[4], ('plonk-host-ragged', r_[0])
        RAN.append(('plonk-host-ragged', r_[0], 0))
    # fixed pv_len device call, the public values at every base offset
    for name, vkey, pv, proof, bad in cases:
        sub = [(vkey, pv, proof, 0)] + ([(vkey, bad, proof, 1)] if bad is not None else []) + [(vkey, pv, proof, 0)]
        n = len(sub)
        d_vk = torch.from_numpy(np.frombuffer(b''.join(x[0] for x in sub), dtype=np.uint8).copy()).cuda()
        d_p = torch.from_numpy(np.frombuffer(b''.join(x[2] for x in sub), dtype=np.uint8).copy()).cuda()
        for k in G.OFFSETS_BYTE:
            keep, p_pv = G.offset_tensor(torch, b''.join(x[1] for x in sub), k)
            d_st = torch.full((n,), 255, dtype=torch.uint8, device='cuda')
            v.verify_batch_dev(n, d_vk.data_ptr(), p_pv, len(pv), d_p.data_ptr(), d_st.data_ptr(), 0, _stream())
            torch.cuda.synchronize()
            assert [int(x) for x in d_st.cpu().numpy()] == [x[3] for x in sub], ('plonk-dev', name, k)
            RAN.append(('plonk-dev', name, k))
    v.close()
    # the PLONK route of a gateway beside the Groth16 route (whose real proof sits first, in the middle and last)
    s = real_proofs['sp1']
    g16 = ('groth16', H(s['vkey']), H(s['public_values']), H(s['proof']), 0)
    mid = len(rows) // 2
    grow = [g16] + rows[:mid] + [g16] + rows[mid:] + [g16]
    gw = zkv.Sp1Gateway(True, [(vkb, h)])
    st, _ = gw.verify_batch([r[1] for r in grow], [r[2] for r in grow], [r[3] for r in grow])
    for r_, x in zip(grow, st):
        assert int(x) == r_[4], ('plonk-gateway', r_[0])
        if r_[0] != 'groth16':
            RAN.append(('plonk-gateway', r_[0], 0))
    gw.close()


# ---------------------------------------------------------------- base offsets of device buffers
def _moved_runs(n_buffers):
    """One buffer moved at a time by 1, 2, 3, then all moved (by 1, 2, 3 in turn round the buffers)."""
    runs = [tuple(0 for _ in range(n_buffers))]
    for b in range(n_buffers):
        for k in G.OFFSETS_BYTE[1:]:
            runs.append(tuple(k if j == b else 0 for j in range(n_buffers)))
    runs.append(tuple(1 + (j % 3) for j in range(n_buffers)))
    return runs


def _runs_for(n_buffers):
    """_moved_runs, then the first buffer (seals / proofs / calldata) alone at 4, 8, 12: still dword-aligned, other 16-byte phases."""
    return _moved_runs(n_buffers) + [tuple(k if j == 0 else 0 for j in range(n_buffers)) for k in G.OFFSETS_WIDE]


def _run_offsets_n(path, inputs, out_sizes, call):
    """inputs: byte strings of the byte-typed device inputs (the first is the seal / proof buffer); out_sizes: bytes of every byte-typed
    output; call(input pointers, output pointers).  Runs every combination of _runs_for over inputs + outputs; returns
    {run: tuple of output bytes}, having checked that the bytes around every output kept their sentinel."""
    import torch
    out = {}
    for run in _runs_for(len(inputs) + len(out_sizes)):
        keeps, ptrs, outs, optrs = [], [], [], []
        for data, k in zip(inputs, run):
            t, p = G.offset_tensor(torch, data, k)
            keeps.append(t); ptrs.append(p)
        for size, k in zip(out_sizes, run[len(inputs):]):
            t, p = G.offset_tensor(torch, bytes([G.SENTINEL]) * size, k)
            outs.append((t, k, size)); optrs.append(p)
        call(ptrs, optrs)
        torch.cuda.synchronize()
        for t, k, size in outs:
            assert G.outside_is_sentinel(t, k, size), (path, run)
        out[run] = tuple(t.cpu().numpy()[k:k + size].tobytes() for t, k, size in outs)
        RAN.append((path, 'offsets', run))
    return out


def _run_offsets(path, inputs, n, call):
    """The same for the entry points with n status bytes and n x 4 received-selector bytes: {run: (status list, recv bytes)}."""
    res = _run_offsets_n(path, inputs, [n, 4 * n], lambda p, o: call(p, o[0], o[1]))
    return {run: (list(v[0]), v[1]) for run, v in res.items()}


def _same_everywhere(path, res, want, want_recv=None):
    base = res[next(iter(res))]
    assert list(base[0]) == list(want), path
    if want_recv is not None:
        assert base[1] == want_recv, path
    for run, got in res.items():
        assert got == base, (path, run)


def test_base_offsets_of_the_single_vm_device_calls(zkv, sp, r0, real_proofs):
    """zkv_risc0_verify_batch_dev, zkv_risc0_verify_integrity_batch_dev and zkv_sp1_verify_batch_dev on 320 proofs (valid, damaged and
    wrong-selector ones): every input and output buffer at base offsets 1, 2, 3, one at a time and all together.  The valid proofs ACCEPT
    in every run, statuses and received selectors equal the aligned run and the oracle, the signals read back equal the aligned run's."""
    from stylus_zkvm_verifiers_amd import synth
    r, s = real_proofs['risc0'], real_proofs['sp1']
    n = 320
    orc = ol.Risc0Oracle(); orc.initialize(H(r['control_root']), H(r['bn254_control_id']))
    seals, mut, _, flip = synth.make_batch('risc0', H(r['seal']), n, 0xB0FF5E71, pool=4, mutate_every=4)
    assert 0 < mut.sum() < n
    ids = np.tile(np.frombuffer(H(r['image_id']), dtype=np.uint8), (n, 1))
    jds = np.tile(np.frombuffer(H(r['journal_digest']), dtype=np.uint8), (n, 1)); jds[flip, 0] ^= 1
    want = [orc.verify(seals[i].tobytes(), ids[i].tobytes(), jds[i].tobytes())[0] for i in range(n)]
    assert want.count(0) >= n // 2 and 5 in want and 1 in want
    sigs = {}

    def call_r0(p, p_st, p_rv):
        r0.verify_batch_dev(n, p[0], p[1], p[2], p_st, p_rv, _stream())
        sigs[len(sigs)] = _signals(r0._h, n)
    _same_everywhere('risc0-dev', _run_offsets('risc0-dev', [seals.tobytes(), ids.tobytes(), jds.tobytes()], n, call_r0), want)
    assert all(v == sigs[0] for v in sigs.values()) and len(sigs) > 10
    # verify_integrity: claim digests
    cl = np.tile(np.frombuffer(H(r['claim_digest']), dtype=np.uint8), (n, 1)); cl[flip, 0] ^= 1
    want_i = [orc.verify_integrity(seals[i].tobytes(), cl[i].tobytes())[0] for i in range(n)]
    assert want_i.count(0) >= n // 2

    def call_r0i(p, p_st, p_rv):
        r0.verify_integrity_batch_dev(n, p[0], p[1], p_st, p_rv, _stream())
    _same_everywhere('risc0-integrity-dev', _run_offsets('risc0-integrity-dev', [seals.tobytes(), cl.tobytes()], n, call_r0i), want_i)
    # SP1
    proofs, mut1, _, flip1 = synth.make_batch('sp1', H(s['proof']), n, 0xB0FF5E72, pool=4, mutate_every=4)
    vk = np.tile(np.frombuffer(H(s['vkey']), dtype=np.uint8), (n, 1))
    pv = np.tile(np.frombuffer(H(s['public_values']), dtype=np.uint8), (n, 1)); pv[flip1, -1] ^= 1
    want_s = [ol.sp1_verify_proof(vk[i].tobytes(), pv[i].tobytes(), proofs[i].tobytes())[0] for i in range(n)]
    assert want_s.count(0) >= n // 2 and 5 in want_s and 1 in want_s
    sigs.clear()

    def call_sp(p, p_st, p_rv):
        sp.verify_batch_dev(n, p[1], p[2], 96, p[0], p_st, p_rv, _stream())
        sigs[len(sigs)] = _signals(sp._h, n)
    _same_everywhere('sp1-dev-offsets', _run_offsets('sp1-dev-offsets', [proofs.tobytes(), vk.tobytes(), pv.tobytes()], n, call_sp), want_s)
    assert all(v == sigs[0] for v in sigs.values()) and len(sigs) > 10


def test_base_offsets_of_the_mixed_and_gateway_device_calls(zkv, real_proofs):
    """zkv_mixed_verify_batch_dev and zkv_sp1_gateway_verify_batch_dev (Groth16 and PLONK routes, ragged proofs): the gather kernels'
    byte paths (mx_ld4 / gw_ld4) run for every moved buffer; statuses and received selectors equal the aligned run and the oracle."""
    from stylus_zkvm_verifiers_amd import parallel, synth
    r, s = real_proofs['risc0'], real_proofs['sp1']
    k0, k1 = 170, 150
    s0, m0, _, f0 = synth.make_batch('risc0', H(r['seal']), k0, 0xB0FF5E73, pool=4, mutate_every=4)
    s1, m1, _, f1 = synth.make_batch('sp1', H(s['proof']), k1, 0xB0FF5E74, pool=4, mutate_every=4)
    ids = np.tile(np.frombuffer(H(r['image_id']), dtype=np.uint8), (k0, 1))
    jds = np.tile(np.frombuffer(H(r['journal_digest']), dtype=np.uint8), (k0, 1)); jds[f0, 0] ^= 1
    vk = np.tile(np.frombuffer(H(s['vkey']), dtype=np.uint8), (k1, 1))
    pv = np.tile(np.frombuffer(H(s['public_values']), dtype=np.uint8), (k1, 1)); pv[f1, -1] ^= 1
    vm, seals, a, b, perm = parallel.interleave([(0, s0, ids, jds), (1, s1, vk, pv)], 0xB0FF5E75)
    n = k0 + k1
    orc = ol.Risc0Oracle(); orc.initialize(H(r['control_root']), H(r['bn254_control_id']))
    want = [orc.verify(seals[i].tobytes(), a[i].tobytes(), b[i, :32].tobytes())[0] if vm[i] == 0
            else ol.sp1_verify_proof(a[i].tobytes(), b[i].tobytes(), seals[i].tobytes())[0] for i in range(n)]
    assert want.count(0) >= n // 2 and 5 in want and 1 in want
    mx = zkv.MixedVerifier(H(r['control_root']), H(r['bn254_control_id']))
    sp_child = zkv._lib.lib().zkv_mixed_ctx_sp1(mx._h)
    i1 = [i for i in range(n) if vm[i] == 1]
    sigs = {}

    def call_mx(p, p_st, p_rv):
        mx.verify_batch_dev(n, p[1], p[0], p[2], p[3], 96, 96, p_st, p_rv, _stream())
        sigs[len(sigs)] = _signals(sp_child, len(i1))
    res = _run_offsets('mixed-dev', [np.ascontiguousarray(seals).tobytes(), np.ascontiguousarray(vm).tobytes(), np.ascontiguousarray(a).tobytes(),
                                     np.ascontiguousarray(b).tobytes()], n, call_mx)
    _same_everywhere('mixed-dev', res, want)
    # read-back inside the compacted slots: the SP1 child's proof j is the j-th SP1 proof of the batch (stable partition)
    sg, fl = sigs[0]
    for j, i in enumerate(i1):
        if fl[j]:
            assert sg[j][1] == G.expected_signal(b[i].tobytes()) and sg[j][0] == int.from_bytes(a[i].tobytes(), 'big'), (j, i)
    assert sum(1 for x in fl if x) >= len(i1) // 2 and all(v == sigs[0] for v in sigs.values())
    mx.close()
    # gateway: Groth16 route + the PLONK route of these tests, ragged proofs
    _, vkb, h = G.plonk_key()
    items = [(vk[j].tobytes(), pv[j].tobytes(), s1[j].tobytes()) for j in range(k1)]
    for name, vkey, pv_, proof, bad in G.plonk_cases():
        if len(pv_) == 96:
            items[3::7] = [(vkey, pv_ if q % 2 == 0 else bad, proof) for q in range(len(items[3::7]))]
    items[5] = (items[5][0], items[5][1], items[5][2][:3])              # short
    items[11] = (items[11][0], items[11][1], b'\x01\x02\x03\x04' + items[11][2][4:])    # no route
    gw = zkv.Sp1Gateway(True, [(vkb, h)])
    ng = len(items)
    want_g, _ = gw.verify_batch([x[0] for x in items], [x[1] for x in items], [x[2] for x in items])
    want_g = [int(x) for x in want_g]
    for (vkey, pv_, proof), w in zip(items, want_g):
        if proof[:4] == h[:4]:
            assert w == ol.sp1_plonk_verify_proof(vkb, h, vkey, pv_, proof)[0]
        elif len(proof) == 260 and proof[:4] == H(s['proof'])[:4]:
            assert w == ol.sp1_verify_proof(vkey, pv_, proof)[0]
    assert want_g.count(0) >= ng // 2 and 4 in want_g and 8 in want_g and 1 in want_g
    off = np.zeros(ng + 1, dtype=np.uint64); off[1:] = np.cumsum([len(x[2]) for x in items])
    import torch
    d_off = torch.from_numpy(off.view(np.int64)).cuda()

    def call_gw(p, p_st, p_rv):
        gw.verify_batch_dev(ng, p[1], p[2], 96, p[0], d_off.data_ptr(), int(off[-1]), p_st, p_rv, _stream())
    res = _run_offsets('gateway-dev', [b''.join(x[2] for x in items), b''.join(x[0] for x in items), b''.join(x[1] for x in items)], ng, call_gw)
    _same_everywhere('gateway-dev', res, want_g)
    gw.close()


def test_base_offsets_of_the_plonk_device_call(zkv):
    """zkv_sp1_plonk_verify_batch_dev on the 96-byte case and its damaged siblings, 192 rows, every buffer moved."""
    vk, vkb, h = G.plonk_key()
    name, vkey, pv, proof, bad = next(c for c in G.plonk_cases() if len(c[2]) == 96)
    rows = []
    for j in range(192):
        q = j % 4
        rows.append((vkey, pv, proof) if q < 2 else (vkey, bad, proof) if q == 2 else (vkey, pv, b'\x00\x00\x00\x07' + proof[4:]))
    want = [ol.sp1_plonk_verify_proof(vkb, h, *x)[0] for x in rows[:4]] * 48
    assert want[:4] == [0, 0, 1, 5]
    v = zkv.Sp1PlonkVerifier(vkb, h)
    n = len(rows)

    def call(p, p_st, p_rv):
        v.verify_batch_dev(n, p[1], p[2], 96, p[0], p_st, p_rv, _stream())
    res = _run_offsets('plonk-dev-offsets', [b''.join(x[2] for x in rows), b''.join(x[0] for x in rows), b''.join(x[1] for x in rows)], n, call)
    _same_everywhere('plonk-dev-offsets', res, want)
    v.close()


def _tile(b, n):
    return np.tile(np.frombuffer(b, dtype=np.uint8), (n, 1))


def test_base_offsets_of_the_risc0_set_and_mixed_call_device_calls(zkv, real_proofs):
    """zkv_risc0_set_verify_batch_dev, zkv_risc0_set_verify_integrity_batch_dev (the uint32 instance indices keep their natural alignment)
    and zkv_mixed_verify_call_batch_dev (the method bytes are one more byte-typed buffer): every byte-typed buffer moved."""
    import torch
    from stylus_zkvm_verifiers_amd import parallel, synth
    r, s = real_proofs['risc0'], real_proofs['sp1']
    rng = random.Random('buffer-geometry-set')
    roots = [H(r['control_root']), rng.randbytes(32)]
    cids = [H(r['bn254_control_id']), rng.randrange(m.R).to_bytes(32, 'big')]
    vs = zkv.RiscZeroVerifierSet(roots, cids)
    oracles = []
    for cr, cid in zip(roots, cids):
        o = ol.Risc0Oracle(); o.initialize(cr, cid); oracles.append(o)
    n = 256
    seals, mut, _, flip = synth.make_batch('risc0', H(r['seal']), n, 0xB0FF5E81, pool=4, mutate_every=4)
    iid = _tile(H(r['image_id']), n)
    jds = _tile(H(r['journal_digest']), n); jds[flip, 0] ^= 1
    cl = _tile(H(r['claim_digest']), n); cl[flip, 0] ^= 1
    inst = np.array([0 if i % 5 else 1 for i in range(n)], dtype=np.uint32)
    for i in range(0, n, 10):                                       # instance 1 under its own selector: reaches the pairing and fails there
        seals[i, :4] = np.frombuffer(oracles[1].get_selector(), dtype=np.uint8)
    inst[17] = 2                                                    # unknown instance
    d_inst = torch.from_numpy(inst.view(np.int32)).cuda()

    def oracle(i, integrity):
        if inst[i] >= 2:
            return 2, bytes(4)
        o = oracles[inst[i]]
        st, rv = (o.verify_integrity(seals[i].tobytes(), cl[i].tobytes()) if integrity
                  else o.verify(seals[i].tobytes(), iid[i].tobytes(), jds[i].tobytes()))
        return st, bytes(rv or bytes(4))
    for integrity in (False, True):
        path = 'risc0-set-integrity-dev' if integrity else 'risc0-set-dev'
        want = [oracle(i, integrity) for i in range(n)]
        assert [w[0] for w in want].count(0) >= n // 2 and {1, 2, 5} <= {w[0] for w in want}

        def call(p, p_st, p_rv):
            if integrity:
                vs.verify_integrity_batch_dev(n, d_inst.data_ptr(), p[0], p[1], p_st, p_rv, _stream())
            else:
                vs.verify_batch_dev(n, d_inst.data_ptr(), p[0], p[1], p[2], p_st, p_rv, _stream())
        inputs = [seals.tobytes(), cl.tobytes()] if integrity else [seals.tobytes(), iid.tobytes(), jds.tobytes()]
        _same_everywhere(path, _run_offsets(path, inputs, n, call), [w[0] for w in want], b''.join(w[1] for w in want))
    vs.close()
    # mixed batch with a method byte per proof
    k0, k1 = 150, 106
    s0, _, _, f0 = synth.make_batch('risc0', H(r['seal']), k0, 0xB0FF5E82, pool=4, mutate_every=4)
    s1, _, _, f1 = synth.make_batch('sp1', H(s['proof']), k1, 0xB0FF5E83, pool=4, mutate_every=4)
    meth0 = np.array([j % 2 for j in range(k0)], dtype=np.uint8)     # verify / verify_integrity alternate
    a0 = np.where(meth0[:, None] == 1, _tile(H(r['claim_digest']), k0), _tile(H(r['image_id']), k0))
    a0[f0 & (meth0 == 1), 0] ^= 1
    b0 = _tile(H(r['journal_digest']), k0); b0[f0 & (meth0 == 0), 0] ^= 1
    vk = _tile(H(s['vkey']), k1)
    pv = _tile(H(s['public_values']), k1); pv[f1, -1] ^= 1
    vm, seals, a, b, perm = parallel.interleave([(0, s0, a0, b0), (1, s1, vk, pv)], 0xB0FF5E84)
    meth = np.concatenate([meth0, np.zeros(k1, dtype=np.uint8)])[perm]
    n = k0 + k1
    i_sp = [i for i in range(n) if vm[i] == 1]
    i_r0 = [i for i in range(n) if vm[i] == 0]
    meth[i_sp[3]] = 1; meth[i_r0[4]] = 2                            # methods the VM does not have
    orc = oracles[0]
    want, want_rv = [], []
    for i in range(n):
        if (vm[i] == 1 and meth[i] != 0) or (vm[i] == 0 and meth[i] > 1):
            st, rv = 6, None
        elif vm[i] == 1:
            st, rv = ol.sp1_verify_proof(a[i].tobytes(), b[i].tobytes(), seals[i].tobytes())
        elif meth[i]:
            st, rv = orc.verify_integrity(seals[i].tobytes(), a[i].tobytes())
        else:
            st, rv = orc.verify(seals[i].tobytes(), a[i].tobytes(), b[i, :32].tobytes())
        want.append(st); want_rv.append(bytes(rv or bytes(4)))
    assert want.count(0) >= n // 2 and {1, 5, 6} <= set(want)
    mx = zkv.MixedVerifier(H(r['control_root']), H(r['bn254_control_id']))

    def call_mx(p, p_st, p_rv):
        mx.verify_batch_dev(n, p[1], p[0], p[2], p[3], 96, 96, p_st, p_rv, _stream(), d_method=p[4])
    res = _run_offsets('mixed-call-dev', [np.ascontiguousarray(x).tobytes() for x in (seals, vm, a, b, meth)], n, call_mx)
    _same_everywhere('mixed-call-dev', res, want, b''.join(want_rv))
    mx.close()


def _pairing_calls(real_proofs):
    """The reference's own 768-byte ecPairing calldata of the real RISC Zero proof (groth16.rs:109-119) and damaged variants of it."""
    r = real_proofs['risc0']
    seal = H(r['seal'])
    w = [seal[4 + 32 * i:36 + 32 * i] for i in range(8)]
    ax, ay = m.negate_g1_words(int.from_bytes(w[0], 'big'), int.from_bytes(w[1], 'big'))
    vk = m.RISC0_VK
    g2 = lambda q: b''.join(m.be32(v) for v in (q[0][0], q[0][1], q[1][0], q[1][1]))
    data = (m.be32(ax) + m.be32(ay) + b''.join(w[2:6]) + m.be32(vk['alpha1'][0]) + m.be32(vk['alpha1'][1]) + g2(vk['beta2'])
            + H(r['vk_x'][0]) + H(r['vk_x'][1]) + g2(vk['gamma2']) + w[6] + w[7] + g2(vk['delta2']))
    bad = bytearray(data); bad[100] ^= 1
    return [data, bytes(bad), bytes(64) + data[64:], data[:64] + bytes(128) + data[192:], data, data[:192] + data[:192] + data[384:], data]


def test_base_offsets_of_the_pairing_and_generic_key_device_calls(zkv, real_proofs):
    """zkv_bn254_pairing_batch_dev (d_in, d_result, d_ok), zkv_groth16_verify_batch_dev, zkv_groth16_set_verify_batch_dev,
    zkv_plonk_verify_batch_dev and zkv_plonk_set_verify_batch_dev (uint32 key indices keep their natural alignment): valid and damaged
    rows, every byte-typed buffer moved; the valid rows verify in every run, the answers equal the aligned run and the oracle."""
    import torch
    import plonk_trapdoor_keys as T
    calls = _pairing_calls(real_proofs) * 32
    n = len(calls)
    exp = [ol.ecpairing(x) for x in calls[:7]] * 32
    want_ok = bytes(0 if e is None else 1 for e in exp)
    assert exp[0] is not None and exp[0][-1] == 1 and None in exp and any(e is not None and e[-1] == 0 for e in exp)
    pc = zkv.Bn254Precompiles()
    res = _run_offsets_n('pairing-dev', [b''.join(calls)], [n, n], lambda p, o: pc.pairing_dev(n, 4, p[0], o[0], o[1], _stream()))
    base = res[next(iter(res))]
    assert base[1] == want_ok and all(base[0][i] == exp[i][-1] for i in range(n) if exp[i] is not None)
    assert all(v == base for v in res.values())
    pc.close()
    # generic Groth16 key and a set of two
    VM = {'risc0': 0, 'sp1': 1}
    rng = random.Random('buffer-geometry-groth16')
    keys, rows = [], []
    for vmn in ('sp1', 'risc0'):
        vk, td = m.trapdoor_vk(rng, 3)
        vkw = m.vk_to_words(vk)
        keys.append((vkw, 3, VM[vmn]))
        for j in range(3):
            sig = [rng.randrange(m.R) for _ in range(2)]
            words = m.proof_to_words(*m.trapdoor_prove(rng, td, sig, vmn))
            sb = b''.join(m.be32(x) for x in sig)
            rows.append((len(keys) - 1, words, sb))
            rows.append((len(keys) - 1, words, sb[:-1] + bytes([sb[-1] ^ 1])))                    # another signal
            rows.append((len(keys) - 1, words[:40] + bytes([words[40] ^ 1]) + words[41:], sb))    # a damaged point
    want = [1 if ol.groth16_verify_vk(keys[k][2], keys[k][0], 3, w_, [sb[:32], sb[32:]]) else 0 for k, w_, sb in rows]
    assert want == [1, 0, 0] * 6
    own = [x for x in rows if x[0] == 0] * 20
    n = len(own)
    v = zkv.Groth16Verifier(keys[0][0], 3, keys[0][2])
    res = _run_offsets_n('groth16-dev', [b''.join(x[1] for x in own), b''.join(x[2] for x in own)], [n],
                         lambda p, o: v.verify_batch_dev(n, p[0], p[1], o[0], _stream()))
    assert all(val == (bytes([1, 0, 0] * (n // 3)),) for val in res.values())
    v.close()
    allr = rows * 12
    n = len(allr)
    gs = zkv.Groth16VerifierSet(keys)
    assert gs.signal_stride() == 64
    d_k = torch.from_numpy(np.array([x[0] for x in allr], dtype=np.uint32).view(np.int32)).cuda()
    res = _run_offsets_n('groth16-set-dev', [b''.join(x[1] for x in allr), b''.join(x[2] for x in allr)], [n],
                         lambda p, o: gs.verify_batch_dev(n, d_k.data_ptr(), p[0], p[1], o[0], _stream()))
    assert all(val == (bytes(want * 12),) for val in res.values())
    gs.close()
    # PLONK key and a set of two
    pkeys, prow = [], []
    for j in range(2):
        vk = T.make_key(T.rng_for('buffer-geometry-plonk-generic-key', j), 2, 1)
        vkb = pm.vk_bytes(vk)
        pkeys.append(vkb)
        prng = T.rng_for('buffer-geometry-plonk-generic-proof', j)
        for q in range(2):
            pub = [prng.randrange(m.R) for _ in range(2)]
            proof = T.forge(vk, pub, prng)
            pb = b''.join(m.be32(x) for x in pub)
            prow.append((j, proof, pb))
            prow.append((j, proof, pb[:-1] + bytes([pb[-1] ^ 1])))
            prow.append((j, proof[:70] + bytes([proof[70] ^ 1]) + proof[71:], pb))
    pwant = [1 if ol.plonk_verify(pkeys[k], T.pad27(pr), [pb[:32], pb[32:]]) else 0 for k, pr, pb in prow]
    assert pwant == [1, 0, 0] * 4 and len(prow[0][1]) == 32 * 27
    own = [x for x in prow if x[0] == 0] * 24
    n = len(own)
    pv_ = zkv.PlonkVerifier(pkeys[0])
    res = _run_offsets_n('plonk-keys-dev', [b''.join(x[1] for x in own), b''.join(x[2] for x in own)], [n],
                         lambda p, o: pv_.verify_batch_dev(n, p[0], p[1], o[0], _stream()))
    assert all(val == (bytes([1, 0, 0] * (n // 3)),) for val in res.values())
    pv_.close()
    allr = prow * 12
    n = len(allr)
    ps = zkv.PlonkVerifierSet(pkeys)
    assert ps.proof_stride() == 32 * 27 and ps.input_stride() == 64
    d_k = torch.from_numpy(np.array([x[0] for x in allr], dtype=np.uint32).view(np.int32)).cuda()
    res = _run_offsets_n('plonk-set-dev', [b''.join(x[1] for x in allr), b''.join(x[2] for x in allr)], [n],
                         lambda p, o: ps.verify_batch_dev(n, d_k.data_ptr(), p[0], p[1], o[0], _stream()))
    assert all(val == (bytes(pwant * 12),) for val in res.values())
    ps.close()


# ---------------------------------------------------------------- placement
PLACEMENT_PATHS = ('sp1', 'mixed', 'mixed-interleaved', 'gateway', 'sp1-dev', 'mixed-dev', 'mixed-interleaved-dev', 'gateway-dev')


def _positions(n):
    """first, middle, last of chunk 0, first of chunk 1 (contexts created with ZKV_CHUNK = 64), last"""
    return (0, n // 2, 63, 64, n - 1)


def test_real_proof_placement_in_ragged_batches(zkv, real_proofs, monkeypatch):
    """The real SP1 proof (96-byte public values) at the first, a middle, the chunk-boundary and the last position of batches whose other
    proofs carry the edge lengths (host calls, ragged) or other 96-byte values (device calls, fixed pv_len): it accepts there and only
    there, through the SP1, mixed (also interleaved with RISC Zero rows) and gateway host and device calls.  The contexts are created
    with 64-proof chunks, so positions 63 and 64 are the last proof of one chunk and the first of the next; the read-back of the last
    chunk (n - 64 proofs; for mixed and gateway contexts from the child that ran them) shows that the batch was split there and that
    the public values of the second chunk were found: the digests inside mixed and gateway slots, at the edge lengths."""
    import torch
    from stylus_zkvm_verifiers_amd import _lib, diag_prep, sp1_gateway
    monkeypatch.setenv('ZKV_CHUNK', '64')
    s, r = real_proofs['sp1'], real_proofs['risc0']
    vkey, proof, real_pv = H(s['vkey']), H(s['proof']), H(s['public_values'])
    seal, iid, jd = H(r['seal']), H(r['image_id']), H(r['journal_digest'])
    base = G.ragged_order(G.messages())
    n = len(base)
    assert 64 < n < 128
    sp = zkv.Sp1Verifier(0)
    mx = zkv.MixedVerifier(H(r['control_root']), H(r['bn254_control_id']))
    gw = zkv.Sp1Gateway(True, [])
    mx_sp = zkv._lib.lib().zkv_mixed_ctx_sp1(mx._h)
    gw_sp = sp1_gateway.lib().zkv_sp1_gateway_route_ctx(gw._h, 0)
    rng = random.Random('buffer-geometry-placement')
    fixed = [rng.randbytes(96) for _ in range(n)]
    buf = np.zeros(64 * 40, dtype=np.uint32)

    def tail_signals(handle, pvs, path):
        """the last chunk holds proofs 64 .. n - 1: one more is refused, and their signals are those of their public values"""
        assert diag_prep.lib().zkv_diag_prep_signals(handle, n - 64 + 1, buf.ctypes.data, buf.ctypes.data) == _lib.ERR_INVALID_ARG, path
        sig, fl = _signals(handle, n - 64)
        for j in range(n - 64):
            assert fl[j] != 0 and sig[j][1] == G.expected_signal(pvs[64 + j]) and sig[j][0] == int.from_bytes(vkey, 'big'), (path, j)

    def dev(x):
        return torch.from_numpy(np.frombuffer(x, dtype=np.uint8).copy()).cuda()
    d_vk, d_p = dev(vkey * n), dev(proof * n)
    off = np.arange(n + 1, dtype=np.uint64) * 260
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    vm2 = [j % 2 for j in range(2 * n)]                               # RISC Zero rows in between: SP1 proof j is row 2 j + 1
    d_vm1, d_vm2 = dev(bytes([1] * n)), dev(bytes(vm2))
    d_seals2 = dev(b''.join(seal if t == 0 else proof for t in vm2))
    d_a2 = dev(b''.join(iid if t == 0 else vkey for t in vm2))
    for pos in _positions(n):
        want = [0 if j == pos else 1 for j in range(n)]
        want2 = [0 if t == 0 else want[j // 2] for j, t in enumerate(vm2)]
        # ---- host calls, ragged public values
        pvs = [pv for _, pv in base]
        pvs[pos] = real_pv
        st, _ = sp.verify_batch([vkey] * n, pvs, [proof] * n)
        assert [int(x) for x in st] == want, ('sp1', pos)
        tail_signals(sp._h, pvs, 'sp1')
        st, _ = mx.verify_batch([1] * n, [proof] * n, [vkey] * n, pvs)
        assert [int(x) for x in st] == want, ('mixed', pos)
        tail_signals(mx_sp, pvs, 'mixed')
        st, _ = mx.verify_batch(vm2, [seal if t == 0 else proof for t in vm2], [iid if t == 0 else vkey for t in vm2],
                                [jd if t == 0 else pvs[j // 2] for j, t in enumerate(vm2)])
        assert [int(x) for x in st] == want2, ('mixed-interleaved', pos)
        tail_signals(mx_sp, pvs, 'mixed-interleaved')
        st, _ = gw.verify_batch([vkey] * n, pvs, [proof] * n)
        assert [int(x) for x in st] == want, ('gateway', pos)
        tail_signals(gw_sp, pvs, 'gateway')
        # ---- device calls, fixed 96-byte public values
        fpv = list(fixed)
        fpv[pos] = real_pv
        d_pv = dev(b''.join(fpv))
        d_st = torch.full((n,), 255, dtype=torch.uint8, device='cuda')
        sp.verify_batch_dev(n, d_vk.data_ptr(), d_pv.data_ptr(), 96, d_p.data_ptr(), d_st.data_ptr(), 0, _stream())
        torch.cuda.synchronize()
        assert [int(x) for x in d_st.cpu().numpy()] == want, ('sp1-dev', pos)
        tail_signals(sp._h, fpv, 'sp1-dev')
        d_st = torch.full((n,), 255, dtype=torch.uint8, device='cuda')
        mx.verify_batch_dev(n, d_vm1.data_ptr(), d_p.data_ptr(), d_vk.data_ptr(), d_pv.data_ptr(), 96, 96, d_st.data_ptr(), 0, _stream())
        torch.cuda.synchronize()
        assert [int(x) for x in d_st.cpu().numpy()] == want, ('mixed-dev', pos)
        tail_signals(mx_sp, fpv, 'mixed-dev')
        d_b2 = dev(b''.join(jd + bytes(64) if t == 0 else fpv[j // 2] for j, t in enumerate(vm2)))
        d_st = torch.full((2 * n,), 255, dtype=torch.uint8, device='cuda')
        mx.verify_batch_dev(2 * n, d_vm2.data_ptr(), d_seals2.data_ptr(), d_a2.data_ptr(), d_b2.data_ptr(), 96, 96, d_st.data_ptr(), 0, _stream())
        torch.cuda.synchronize()
        assert [int(x) for x in d_st.cpu().numpy()] == want2, ('mixed-interleaved-dev', pos)
        tail_signals(mx_sp, fpv, 'mixed-interleaved-dev')
        d_st = torch.full((n,), 255, dtype=torch.uint8, device='cuda')
        gw.verify_batch_dev(n, d_vk.data_ptr(), d_pv.data_ptr(), 96, d_p.data_ptr(), d_off.data_ptr(), 260 * n, d_st.data_ptr(), 0, _stream())
        torch.cuda.synchronize()
        assert [int(x) for x in d_st.cpu().numpy()] == want, ('gateway-dev', pos)
        tail_signals(gw_sp, fpv, 'gateway-dev')
        for path in PLACEMENT_PATHS:
            RAN.append(('placement-' + path, 'real', pos))
    sp.close(); mx.close(); gw.close()


# ---------------------------------------------------------------- the record
def _generated():
    names = [n for n, _ in G.messages()]
    cells = set()
    for n_ in names:
        cells.add(('sp1-host-ragged', n_, 0)); cells.add(('sp1-wire', n_, 0))
        for k in G.OFFSETS_BYTE:
            cells.add(('sp1-dev', n_, k)); cells.add(('plonk-dev', n_, k))
        for suffix in ('', '-flipped'):
            if suffix and n_ == 'rand0':
                continue
            cells.add(('plonk-host-ragged', n_ + suffix, 0)); cells.add(('plonk-gateway', n_ + suffix, 0))
    for k in G.OFFSETS_BYTE + G.OFFSETS_WIDE:
        cells.add(('wire-dev-sp1', 'blob', k)); cells.add(('wire-dev-risc0', 'blob', k))
    cells.add(('risc0-claim', 'pairs', 0)); cells.add(('risc0-claim', 'integrity', 0))
    for path, nb in (('risc0-dev', 3), ('risc0-integrity-dev', 2), ('sp1-dev-offsets', 3), ('mixed-dev', 4), ('gateway-dev', 3), ('plonk-dev-offsets', 3)):
        for run in _runs_for(nb + 2):
            cells.add((path, 'offsets', run))
    for path, nb in (('risc0-set-dev', 3), ('risc0-set-integrity-dev', 2), ('mixed-call-dev', 5)):
        for run in _runs_for(nb + 2):
            cells.add((path, 'offsets', run))
    for path, nb in (('pairing-dev', 3), ('groth16-dev', 3), ('groth16-set-dev', 3), ('plonk-keys-dev', 3), ('plonk-set-dev', 3)):
        for run in _runs_for(nb):                                     # inputs and outputs together
            cells.add((path, 'offsets', run))
    n = len(G.ragged_order(G.messages()))
    for path in PLACEMENT_PATHS:
        for pos in _positions(n):
            cells.add(('placement-' + path, 'real', pos))
    return cells


def test_every_generated_cell_ran(zkv):
    """Runs last: every cell the generators define was run (and passed) above, none was skipped or sampled; the misaligned wire records
    cover every message at some residue and every residue; and no kernel of this module left a wait fault behind."""
    ran = set(RAN)
    gen = _generated()
    mis = {c for c in ran if c[0] == 'sp1-wire-misaligned'}
    assert {c[1] for c in mis} == {n for n, _ in G.messages()} and {c[2] for c in mis} == {0, 1, 2, 3}
    ran -= mis
    assert ran == gen, (sorted(gen - ran, key=str)[:10], sorted(ran - gen, key=str)[:10])
    assert len(ran) == len(gen) and len(gen) > 500
    faults = C.c_uint64(1)
    assert zkv._lib.lib().zkv_diag_wait_faults(0, C.byref(faults)) == 0 and faults.value == 0
