"""The walk-prefix cache of an SP1 context (csrc/zkv_gt.h: k_gt_cache_fill, k_gt_cache_tag, the hit path of final_exp_prog_p) on the device,
lane pairs forced, n = 70 (two full wavefronts and a partial one).  Every case runs the same calls on a context with the cache and on one
with ZKV_GT_CACHE=0 in the same build and compares the status bytes and the walk's product (zkv_diag_gt_product, canonical form); the
statuses are also those of the construction: 0 only for the real proof with its own vkey and public values."""
import random

import numpy as np
import pytest

import spec_model as m

pytestmark = pytest.mark.gpu

H = bytes.fromhex
N = 70
K = 4                                              # GT_CACHE_ENTRIES


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


def sample_positions(n):
    cnt = min(n, 32)
    return [k * n // cnt for k in range(cnt)]


def vkeys(seed, count):
    rng = random.Random(seed)
    return [rng.randrange(1, m.R).to_bytes(32, 'big') for _ in range(count)]


def flipped(b, i):
    p = bytearray(b)
    p[(7 * i) % len(p)] ^= 1 << (i % 8)
    return bytes(p)


class Batch:
    """n rows of the real SP1 proof with the given vkeys; rows in `bad_pv` get one flipped public-values byte, rows in `bad_proof` one
    flipped proof byte (behind the selector).  want: 0 where the row is the untouched real proof, otherwise nonzero."""
    def __init__(self, s, keys, bad_pv=(), bad_proof=()):
        real_vk, pv, proof = H(s['vkey']), H(s['public_values']), H(s['proof'])
        self.keys = list(keys)
        self.pvs = [flipped(pv, i) if i in bad_pv else pv for i in range(len(keys))]
        self.proofs = [proof[:40] + bytes([proof[40] ^ 1]) + proof[41:] if i in bad_proof else proof for i in range(len(keys))]
        self.ok = [k == real_vk and i not in bad_pv and i not in bad_proof for i, k in enumerate(keys)]
        self.signals = [(int.from_bytes(k, 'big'), m.sp1_hash_public_values(p)) for k, p in zip(self.keys, self.pvs)]


def run_both(zkv, monkeypatch, calls):
    """calls: Batch objects (verify) or lists of (s0, s1) (zkv_diag_gt_product), in order, on a fresh context with the cache and on a fresh
    one without.  Returns the cache's counters after every call on the first; asserts that both give the same results."""
    from stylus_zkvm_verifiers_amd import diag_gt
    monkeypatch.delenv('ZKV_GT_WINDOW_BITS', raising=False)
    monkeypatch.delenv('ZKV_GT_MAX_BYTES', raising=False)
    out, counters = {}, []
    for mode in ('1', '0'):
        monkeypatch.setenv('ZKV_GT_CACHE', mode)
        v = zkv.Sp1Verifier()
        try:
            v.set_lanes_per_proof(2)
            res = []
            for c in calls:
                if isinstance(c, Batch):
                    st, rv = v.verify_batch(c.keys, c.pvs, c.proofs)
                    st = [int(x) for x in st]
                    assert [x == 0 for x in st] == c.ok, (mode, len(res), st)
                    res.append((st, np.asarray(rv).tolist()))
                else:
                    res.append(diag_gt.product(v._h, c))
                state = diag_gt.cache(v._h)
                if mode == '1':
                    counters.append(state)
                else:
                    assert state == dict(valid=0, fills=0, entries=0)
            assert diag_gt.info(v._h)['built']
            out[mode] = res
        finally:
            v.close()
    for i, (a, b) in enumerate(zip(out['1'], out['0'])):
        assert a == b, ('call', i)
    assert all(c['entries'] == K for c in counters)
    return counters


def test_one_vkey_cold_then_warm(zkv, monkeypatch, real_proofs):
    s = real_proofs['sp1']
    b = Batch(s, [H(s['vkey'])] * N, bad_pv=set(range(2, N, 3)))
    got = run_both(zkv, monkeypatch, [b, b, b.signals])
    assert [(c['valid'], c['fills']) for c in got] == [(1, 1)] * 3


def test_two_vkeys_alternating_and_mutated_proofs(zkv, monkeypatch, real_proofs):
    """Proof by proof: every wavefront of the first call holds hit lanes (the real vkey, inserted by that call) beside miss lanes; the second call
    inserts the other vkey, from the third on every lane hits."""
    s = real_proofs['sp1']
    other = vkeys(2, 1)[0]
    keys = [H(s['vkey']) if i % 2 == 0 else other for i in range(N)]
    pos = sample_positions(N)
    assert sum(p % 2 == 0 for p in pos) >= 2 and sum(p % 2 for p in pos) >= 2 and pos[0] == 0
    b = Batch(s, keys, bad_pv={4, 33, 64}, bad_proof={10, 66})
    got = run_both(zkv, monkeypatch, [b, b.signals, b, b.signals, b, b.signals])
    assert [(c['valid'], c['fills']) for c in got] == [(1, 1), (2, 2), (2, 2), (2, 2), (2, 2), (2, 2)]


def test_distinct_vkeys_insert_nothing(zkv, monkeypatch, real_proofs):
    s = real_proofs['sp1']
    keys = vkeys(3, N)
    keys[5] = H(s['vkey'])                          # one accepted proof among them
    assert len(set(keys)) == N
    b = Batch(s, keys)
    got = run_both(zkv, monkeypatch, [b, b.signals, b])
    assert [(c['valid'], c['fills']) for c in got] == [(0, 0)] * 3


def test_eviction_over_successive_calls(zkv, monkeypatch, real_proofs):
    """K + 1 vkeys, one per call: the fifth insertion wraps the cursor and evicts the first (the real vkey), which the next call inserts
    again over the second; the third is still cached when it comes back."""
    s = real_proofs['sp1']
    ks = [H(s['vkey'])] + vkeys(4, K)
    calls = [Batch(s, [k] * N, bad_pv={1, 69}) for k in ks]
    calls += [calls[0], calls[0].signals, calls[2], calls[1]]
    got = run_both(zkv, monkeypatch, calls)
    assert [(c['valid'], c['fills']) for c in got] == [(1, 1), (2, 2), (3, 3), (4, 4), (4, 5), (4, 6), (4, 6), (4, 6), (4, 7)]


def test_special_scalars(zkv, monkeypatch, real_proofs):
    """Signal 0 = 0 (u = 1 is what gets cached), 1, 2^19 (the largest digit), 2^20 - 1 (digit -1 and a carry into the next window) and R - 1,
    the largest value PREP accepts: each as a batch of its own, cold and warm, then all of them mixed with random signals in one batch --
    five repeated keys against four slots."""
    s = real_proofs['sp1']
    rng = random.Random(5)
    special = [0, 1, 1 << 19, (1 << 20) - 1, m.R - 1]
    calls = [Batch(s, [H(s['vkey'])] * N)]         # the context's first verify call builds the tables
    for x in special:
        rows = [(x, rng.randrange(m.R)) for _ in range(N)]
        calls += [rows, rows]
    mixed = [(special[i % 7], rng.randrange(m.R)) if i % 7 < 5 else (rng.randrange(m.R), rng.randrange(m.R)) for i in range(N)]
    calls += [mixed, mixed, mixed]
    got = run_both(zkv, monkeypatch, calls)
    fills = [c['fills'] for c in got]
    assert fills[:11] == [1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6]
    # by then 2^20 - 1 and R - 1 have wrapped the cursor over the real vkey and 0: the first mixed call finds 0 absent and repeated (rows 0, 28,
    # 35, ... are sampled) and inserts it; one insertion per call at most
    assert all(0 <= b - a <= 1 for a, b in zip(fills[10:], fills[11:])) and fills[11] == fills[10] + 1
    assert all(c['valid'] == min(c['fills'], K) for c in got)


def test_vkey_out_of_range_is_never_inserted(zkv, monkeypatch, real_proofs):
    """vkey = R and vkey = 2^256 - 1 at sampled positions, several times each: PREP rejects them (dead proofs, their scalar rows are stale),
    so they are no samples.  The first call leaves rows behind, the second has the bad vkeys, the third the real vkey twice among the
    samples beside them: only that one is inserted."""
    s = real_proofs['sp1']
    pos = sample_positions(N)
    bad = [m.R.to_bytes(32, 'big'), b'\xff' * 32]
    first = Batch(s, vkeys(6, N))
    keys = vkeys(7, N)
    for k, p in enumerate(pos[:8]):
        keys[p] = bad[k % 2]
    second = Batch(s, keys)
    keys = list(keys)
    keys[pos[10]] = keys[pos[20]] = H(s['vkey'])
    third = Batch(s, keys)
    got = run_both(zkv, monkeypatch, [first, second, second, third, third])
    assert [(c['valid'], c['fills']) for c in got] == [(0, 0), (0, 0), (0, 0), (1, 1), (1, 1)]


def test_smaller_batch_after_the_cache_was_built(zkv, monkeypatch, real_proofs):
    s = real_proofs['sp1']
    big = Batch(s, [H(s['vkey'])] * N, bad_pv={3})
    small = Batch(s, [H(s['vkey'])] * 33, bad_pv={0, 32})
    got = run_both(zkv, monkeypatch, [big, small, small.signals, big.signals])
    assert [(c['valid'], c['fills']) for c in got] == [(1, 1)] * 4
