"""The aggregate check on Groth16 key sets (include/zkv_groth16_set.h): the same device-resident batch with the
check off and on.

    python tools/bench_groth16_key_sets_aggregate.py [--cases mixed16,long129,short3] [--log2n 18] [--steps 3] [--damaged 0|1|both]

One JSON line per case and batch kind; best of --steps timed calls after a warm-up call; the verdicts with the check on must equal the
ones with it off.  The check runs at the automatic size with an OS-drawn secret and the default ZKV_AGG_MIN.
  mixed16  16 keys, n_ic in {2, 3, 5, 7, 9, 17}, 2^log2n shuffled proofs: the set with the check off against on
  long129  a 1-key set with n_ic = 129, 2^log2n proofs: off against on
  short3   a 1-key set with n_ic = 3 and the check on against Groth16Verifier on the same key with the check on (the short-key sums form)
damaged 1: one proof in 64 damaged, a fifth of those (a wrong last signal) rejected at the pairing, the rest before it (a signal equal to
r, C off the curve, B outside the subgroup).  Proofs: one trapdoor proof per key re-randomised into 4,096 distinct ones, tiled.
Not bench.py.
"""
import argparse
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from bench_groth16_key_sets import VM, m, set_call, single_call, synth, timed, zkv      # noqa: E402

DAMAGE = ('signal_last', 'signal_eq_r', 'c_off_curve', 'b_out_of_subgroup', 'signal_eq_r')


def key_batch(rng, n_ic, vm, count, seed, damaged):
    vk, td = m.trapdoor_vk(rng, n_ic)
    sig = [rng.randrange(m.R) for _ in range(n_ic - 1)]
    base = m.proof_to_words(*m.trapdoor_prove(rng, td, sig, vm))
    vkb = m.vk_to_words(vk)
    p, s, bad, _ = synth.make_groth16_batch(vkb, vm, base, sig, count, seed=seed, mutate_every=64 if damaged else 1 << 30, classes=DAMAGE)
    return (vkb, n_ic, VM[vm]), p, s, bad


def tile(a, n):
    return np.tile(a, (n // len(a),) + (1,) * (a.ndim - 1))


def off_on(s, kk, p, sg, steps):
    s.set_aggregate_check(False)
    ms_off, want = set_call(s, kk, p, sg, steps)
    c0 = s.aggregate_counters()
    s.set_aggregate_check(True)
    ms_on, got = set_call(s, kk, p, sg, steps)
    c1 = s.aggregate_counters()
    assert (got == want).all(), int((got != want).sum())
    return ms_off, ms_on, want, (c1[0] - c0[0], c1[1] - c0[1]), s.last_stage_ms()


def case_mixed16(n, steps, damaged):
    rng = random.Random(16)
    per = n // 16
    keys, ps, ss = [], [], []
    for j in range(16):
        key, p, sg, _ = key_batch(rng, (2, 3, 5, 7, 9, 17)[j % 6], 'risc0' if j % 2 else 'sp1', 4096, 100 + j, damaged)
        keys.append(key); ps.append(tile(p, per)); ss.append(tile(sg, per))
    kk = np.repeat(np.arange(16, dtype=np.uint32), per)
    sigs = np.zeros((n, 16, 32), np.uint8)
    for j, sg in enumerate(ss):
        sigs[per * j:per * (j + 1), :sg.shape[1]] = sg
    perm = np.random.default_rng(0).permutation(n)
    s = zkv.Groth16VerifierSet(keys)
    off, on, want, cnt, st = off_on(s, kk[perm], np.concatenate(ps)[perm], sigs[perm], steps)
    s.close()
    return dict(case='mixed16', n=n, damaged=damaged, off_ms=off, on_ms=on, ratio=on / off, accepted=int(want.sum()),
                sub_batches=cnt[0], failed_sub_batches=cnt[1], on_stage_ms=st)


def case_long129(n, steps, damaged):
    key, p, sg, _ = key_batch(random.Random(129), 129, 'sp1', 4096, 7, damaged)
    s = zkv.Groth16VerifierSet([key])
    off, on, want, cnt, st = off_on(s, np.zeros(n, np.uint32), tile(p, n), tile(sg, n), steps)
    s.close()
    return dict(case='long129', n=n, damaged=damaged, off_ms=off, on_ms=on, ratio=on / off, accepted=int(want.sum()),
                sub_batches=cnt[0], failed_sub_batches=cnt[1], on_stage_ms=st)


def case_short3(n, steps, damaged):
    key, p, sg, _ = key_batch(random.Random(3), 3, 'sp1', 4096, 3, damaged)
    p, sg = tile(p, n), tile(sg, n)
    s = zkv.Groth16VerifierSet([key])
    s.set_aggregate_check(True)
    c0 = s.aggregate_counters()
    ms_set, out = set_call(s, np.zeros(n, np.uint32), p, sg, steps)
    c1 = s.aggregate_counters()
    st = s.last_stage_ms()
    s.close()
    v = zkv.Groth16Verifier(*key)
    v.set_aggregate_check(True)
    fn, d_v = single_call(v, p, sg, steps)
    ms_one = timed(fn, steps)
    assert (d_v.cpu().numpy() == out).all()
    v.close()
    return dict(case='short3', n=n, damaged=damaged, set_on_ms=ms_set, groth16_verifier_on_ms=ms_one, ratio=ms_set / ms_one,
                accepted=int(out.sum()), sub_batches=c1[0] - c0[0], failed_sub_batches=c1[1] - c0[1], on_stage_ms=st)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='mixed16,long129,short3')
    ap.add_argument('--log2n', type=int, default=18)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--damaged', default='both', choices=['0', '1', 'both'])
    args = ap.parse_args()
    if zkv.device_count() < 1:
        sys.exit('no gfx950 device')
    kinds = [False, True] if args.damaged == 'both' else [args.damaged == '1']
    fns = {'mixed16': case_mixed16, 'long129': case_long129, 'short3': case_short3}
    for c in args.cases.split(','):
        for d in kinds:
            print(json.dumps(fns[c](1 << args.log2n, args.steps, d)), flush=True)


if __name__ == '__main__':
    main()
