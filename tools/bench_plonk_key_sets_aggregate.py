"""The aggregate check on PLONK key sets (include/zkv_plonk_set_agg.h) against the parent commit.

    python tools/bench_plonk_key_sets_aggregate.py --parent DIR [--cases one_class,four_classes,one_key,many,off] [--log2n 18] [--steps 3] [--out FILE]

DIR holds the parent commit's package (DIR/stylus_zkvm_verifiers_amd with its built library): a set of the parent ignores the check, so its
verify_batch_dev is the per-proof time.  Both libraries live in this process and the variants of a case run alternately, each timed
--steps times after a warm-up call; the best and the spread (worst - best) of each are reported, and every verdict is checked.  Every case
runs on valid proofs and on the "one in 64 damaged, a fifth of those at the pairing" batch.  Device-resident batches (torch tensors).
  one_class     16 keys of one SRS class, 2^log2n shuffled proofs: the check on, against the parent's set call; with the parent's Miller and
                final-exponentiation stage times (the target: faster by at least half their sum on valid proofs)
  four_classes  16 keys in 4 classes of 4, the same
  one_key       a 1-key set with the check on against the parent's PlonkVerifier with the check on (and both with it off)
  many          256 keys x 16 proofs of one class, ZKV_AGG_MIN lowered to 64: reported, no target (a quarter of every sub-batch is live)
  off           this commit's set with the check off against the parent's set call, 16 keys of one class: the off path must not have moved
Not bench.py.  PARITY UNPINNED BY CONSTRUCTION (no PLONK in the reference).
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import plonk_shared_srs as S                             # noqa: E402
import stylus_zkvm_verifiers_amd as zkv                  # noqa: E402

SHAPES = [(0, 0), (2, 1), (9, 0), (3, 1)]


def load_parent(d):
    """The parent commit's package under the name zkv_parent (its own library: _lib resolves it next to the package's files)."""
    init = os.path.join(d, 'stylus_zkvm_verifiers_amd', '__init__.py')
    spec = importlib.util.spec_from_file_location('zkv_parent', init, submodule_search_locations=[os.path.dirname(init)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules['zkv_parent'] = mod
    spec.loader.exec_module(mod)
    return mod


def race(fns, steps):
    import torch
    for f in fns:
        f()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(steps):
        for k, f in enumerate(fns):
            torch.cuda.synchronize()
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t) * 1e3)
    return [min(t) for t in times], [max(t) - min(t) for t in times]


def to_dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def keys_of(classes, per_class):
    """per_class keys in each of `classes` SRS classes, shapes cycling: [(class, nb, nc, tag)]."""
    return [('bench%d' % c, SHAPES[t % 4][0], SHAPES[t % 4][1], t) for c in range(classes) for t in range(per_class)]


def batch(keys, kk, ps, ins, damaged, seed):
    """Rows of the set's strides for key indices kk, from 2 forged proofs per key; damaged: one row in 64 is damaged, a fifth of those at the
    pairing (the claimed l(zeta) plus one), the others by a scalar >= R.  -> proofs, inputs, expected verdicts."""
    n = len(kk)
    j = np.random.default_rng(seed).integers(0, 2, n)
    proofs = np.zeros((n, ps), np.uint8)
    pub = np.zeros((n, max(ins // 32, 1), 32), np.uint8)
    for b, k in enumerate(keys):
        P, Q = S.rows_of(*k, 2, ps, ins)
        m = kk == b
        proofs[m] = P[j[m]]
        if Q.shape[1]:
            pub[m, :Q.shape[1]] = Q[j[m]]
    want = np.ones(n, np.uint8)
    if damaged:
        bad = np.arange(63, n, 64)
        want[bad] = 0
        S.damage_at_the_pairing(proofs, bad[::5])
        early = np.setdiff1d(bad, bad[::5])
        proofs[early, 12 * 32:13 * 32] = 0xFF                                   # l(zeta) >= R
    return proofs, pub, want


def set_fn(s, kk, proofs, pub):
    import torch
    n = len(kk)
    d_k, d_p, d_i = to_dev(kk.view(np.int32), proofs, pub)
    d_v = torch.zeros(n, dtype=torch.uint8, device='cuda')
    return (lambda: s.verify_batch_dev(n, d_k.data_ptr(), d_p.data_ptr(), d_i.data_ptr(), d_v.data_ptr())), d_v


def single_fn(v, P, Q):
    import torch
    n = len(P)
    d_p, = to_dev(P)
    d_i = to_dev(Q)[0] if Q.size else None
    d_v = torch.zeros(n, dtype=torch.uint8, device='cuda')
    return (lambda: v.verify_batch_dev(n, d_p.data_ptr(), d_i.data_ptr() if d_i is not None else 0, d_v.data_ptr())), d_v


def set_case(name, keys, kk, args, parent, check=True):
    vks = [S.key_bytes(*k) for k in keys]
    out = []
    for damaged in (False, True):
        new, old = zkv.PlonkVerifierSet(vks), parent.PlonkVerifierSet(vks)
        proofs, pub, want = batch(keys, kk, new.proof_stride(), new.input_stride(), damaged, 7)
        if check:
            new.set_aggregate_check(True)
        f_new, o_new = set_fn(new, kk, proofs, pub)
        f_old, o_old = set_fn(old, kk, proofs, pub)
        # the parent twice per round: the difference between its two columns is the spread of one variant against itself
        (ms_new, ms_old, ms_old2), (sp_new, sp_old, sp_old2) = race([f_new, f_old, f_old], args.steps)
        f_new(); st_new = new.last_stage_ms()
        f_old(); st_old = old.last_stage_ms()
        assert np.array_equal(o_new.cpu().numpy(), want) and np.array_equal(o_old.cpu().numpy(), want)
        r = dict(case=name, damaged=damaged, n=len(kk), keys=len(keys), classes=new.srs_classes()[1], check=check, this_ms=ms_new, parent_ms=ms_old,
                 parent_again_ms=ms_old2, spread_ms=[sp_new, sp_old, sp_old2], ratio=ms_new / ms_old, this_stage_ms=st_new, parent_stage_ms=st_old,
                 parent_miller_plus_finalexp_ms=st_old[3] + st_old[4], saved_ms=ms_old - ms_new, counters=new.aggregate_counters())
        if check and not damaged and name in ('one_class', 'four_classes'):
            r['target_saved_ms'] = 0.5 * (st_old[3] + st_old[4])
            r['target_met'] = bool(ms_old - ms_new >= r['target_saved_ms'])
        new.close(); old.close()
        out.append(r)
    return out


def case_one_class(args, parent):
    n = 1 << args.log2n
    return set_case('one_class', keys_of(1, 16), np.random.default_rng(16).integers(0, 16, n).astype(np.uint32), args, parent)


def case_four_classes(args, parent):
    n = 1 << args.log2n
    return set_case('four_classes', keys_of(4, 4), np.random.default_rng(17).integers(0, 16, n).astype(np.uint32), args, parent)


def case_off(args, parent):
    n = 1 << args.log2n
    return set_case('off', keys_of(1, 16), np.random.default_rng(16).integers(0, 16, n).astype(np.uint32), args, parent, check=False)


def case_many(args, parent):
    os.environ['ZKV_AGG_MIN'] = '64'
    keys = [('bench0', SHAPES[t % 4][0], SHAPES[t % 4][1], t % 8) for t in range(256)]      # 8 distinct keys listed 32 times: separate tables each
    kk = np.random.default_rng(1).permutation(np.repeat(np.arange(256, dtype=np.uint32), 16))
    try:
        return set_case('many', keys, kk, args, parent)
    finally:
        del os.environ['ZKV_AGG_MIN']


def case_one_key(args, parent):
    n = 1 << args.log2n
    key = ('bench0', 2, 1, 1)
    vk = S.key_bytes(*key)
    out = []
    for damaged in (False, True):
        s, v = zkv.PlonkVerifierSet([vk]), parent.PlonkVerifier(vk)
        proofs, pub, want = batch([key], np.zeros(n, np.uint32), s.proof_stride(), s.input_stride(), damaged, 9)
        f_set, o_set = set_fn(s, np.zeros(n, np.uint32), proofs, pub)
        f_one, o_one = single_fn(v, proofs, pub)
        (off_set, off_one), _ = race([f_set, f_one], args.steps)
        s.set_aggregate_check(True); v.set_aggregate_check(True)
        (on_set, on_one, on_one2), spread = race([f_set, f_one, f_one], args.steps)
        f_set(); st_set = s.last_stage_ms()
        f_one(); st_one = v.last_stage_ms()
        assert np.array_equal(o_set.cpu().numpy(), want) and np.array_equal(o_one.cpu().numpy(), want)
        out.append(dict(case='one_key', damaged=damaged, n=n, set_on_ms=on_set, plonk_verifier_on_ms=on_one, plonk_verifier_on_again_ms=on_one2, spread_ms=spread,
                        ratio_on=on_set / on_one, set_off_ms=off_set, plonk_verifier_off_ms=off_one, ratio_off=off_set / off_one, set_stage_ms=st_set,
                        plonk_verifier_stage_ms=st_one, counters=s.aggregate_counters()))
        s.close(); v.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True)
    ap.add_argument('--cases', default='one_class,four_classes,one_key,many,off')
    ap.add_argument('--log2n', type=int, default=18)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    torch.zeros(1).cuda()
    parent = load_parent(args.parent)
    fns = dict(one_class=case_one_class, four_classes=case_four_classes, one_key=case_one_key, many=case_many, off=case_off)
    for c in args.cases.split(','):
        for r in fns[c](args, parent):
            line = json.dumps(r)
            print(line, flush=True)
            if args.out:
                with open(args.out, 'a') as f:
                    f.write(line + '\n')


if __name__ == '__main__':
    main()
