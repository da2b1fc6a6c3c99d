"""Valid proofs that reach the point-at-infinity and zero-scalar branches (tests/degenerate_cases.py), and their one-value siblings, on
the CPU: the spec model, the PLONK model and the C oracle must agree (valid accepted, sibling rejected), and so must the host builds of
the kernels' own stage functions -- all three Groth16 mappings (one value per lane, lane pairs, 16 lanes and one / two wavefronts per
proof), the long-key walk, and the generic PLONK pre-pairing stage.  Before these cases every degenerate input of the suite was one to
REJECT, which a kernel computing garbage on such a branch also does."""
import ctypes as C

import degenerate_cases as D
import plonk_model as pm
import spec_model as m
from test_groth16_long_keys import hsl  # noqa: F401  (fixture)
from test_kernel_math_host import hs, hs_pair, hs_wide  # noqa: F401  (fixtures)
from test_plonk_keys_host import host_verdict, hspk  # noqa: F401  (fixture)


def _sig(sig):
    return b''.join(m.be32(s) for s in sig) + b'\0'


def _check_models(cases, model):
    bad = []
    for c in cases:
        want = c[-1]
        got = model(c)
        if got != (want, want):
            bad.append((c[0], want, got))
    assert not bad, bad


def test_groth16_cases_reach_both_oracles():
    cases = D.short_cases() + D.long_cases()
    assert sum(1 for c in cases if c[-1]) == sum(1 for c in cases if not c[-1]) >= 90
    _check_models(cases, D.g16_model)


def _prepare(hs, case):
    name, vm, vk, vkb, words, sig, _ = case
    hs.hs_prepare_generic.restype = C.c_void_p
    fl = C.c_uint32(0); norm = (C.c_uint32 * 48)(); b = (C.c_uint32 * 32)()
    t = hs.hs_prepare_generic(vkb, len(vk['ic']), 1 if vm == 'risc0' else 0, words, _sig(sig), C.byref(fl), norm, b)
    return t, fl.value, norm, b


def test_groth16_short_keys_on_every_host_mapping(hs, hs_pair, hs_wide):
    """One value per lane (hs_groth16_generic), lane pairs (hs2_pairing), 16 lanes (hs3_pairing): every case and sibling.  One and two
    wavefronts per proof (hs3_pairing_w64 / _w64d, 48 and 96 host threads) on the n_ic = 3 cases."""
    bad = []
    seen = set()
    for case in D.short_cases():
        name, vm, vk, vkb, words, sig, want = case
        n_ic = len(vk['ic'])
        got = {'lane': hs.hs_groth16_generic(vkb, n_ic, 1 if vm == 'risc0' else 0, words, _sig(sig))}
        t, fl, norm, b = _prepare(hs, case)
        assert t, name                                   # every case reaches the pairing: only the pairing check may reject
        sub = C.c_int(0)
        got['pair'] = hs_pair.hs2_pairing(t, fl, norm, b, C.byref(sub))
        got['wide16'] = hs_wide.hs3_pairing(t, fl, norm, b)
        kind = (name.split(' / ')[0], n_ic == 3)
        if kind[1] and kind not in seen:
            got['w64'] = hs_wide.hs3_pairing_w64(t, fl, norm, b)
            got['w64d'] = hs_wide.hs3_pairing_w64d(t, fl, norm, b)
            if not want:
                seen.add(kind)
        for k, v in got.items():
            if v != int(want):
                bad.append((name, k, v))
    assert not bad, bad
    assert len(seen) >= 10


def test_groth16_long_keys_on_the_long_key_walk(hsl):
    """The long-key PREP / MSM (the walk sliced over 1, 16 and 64 lanes) and the pairing stages: n_ic = 9 and 129."""
    bad = []
    for name, vm, vk, vkb, words, sig, want in D.long_cases():
        for lanes in (1, 16, 64):
            got = hsl.hsl_verify(vkb, len(vk['ic']), 1 if vm == 'risc0' else 0, words, _sig(sig), lanes)
            if got != int(want):
                bad.append((name, lanes, got))
    assert not bad, bad


def test_plonk_cases_reach_both_oracles():
    cases = D.plonk_cases()
    assert sum(1 for c in cases if c[-1]) == sum(1 for c in cases if not c[-1]) == len(D.PLONK_SPECS)
    _check_models(cases, D.plonk_model)


def test_plonk_cases_on_the_host_prepare_stage(hspk):
    """plonk_prepare for any key (the code of k_plonk_prep_keys), then the two-pair check through the C oracle's ecPairing."""
    bad = []
    for name, nb, nc, vk, vkb, proof, pub, want in D.plonk_cases():
        got = host_verdict(hspk, vkb, proof, [x.to_bytes(32, 'big') for x in pub])
        if got != int(want):
            bad.append((name, got))
    assert not bad, bad


def test_sp1_plonk_cases_on_models_and_host_stage(hspk):
    """SP1 PLONK keys (two public inputs: program vkey and sha256(pv) & (2^253 - 1); one commitment): both oracles' statuses, and the
    host stage on the proof after its selector."""
    bad = []
    n = 0
    for vkb, cases in D.sp1_plonk_cases().items():
        for name, vk, vkey, pv, proof, want in cases:
            status = pm.OK if want else pm.VERIFICATION_FAILED
            got = D.sp1_model(vk, vkey, pv, proof)
            pub = [vkey, m.be32(m.sp1_hash_public_values(pv))]
            host = host_verdict(hspk, vkb, proof[4:], pub)
            if got != (status, status) or host != int(want):
                bad.append((name, got, host))
            n += 1
    assert not bad, bad
    assert n == 2 * len(D.SP1_SPECS) >= 10
