"""Throughput of PLONK key sets (include/zkv_plonk_set.h) against per-key PlonkVerifier contexts.

    python tools/bench_plonk_key_sets.py [--cases one,mixed16,many,setup] [--log2n 18] [--steps 3] [--out FILE]

One JSON line per case (printed, and appended to --out when given); device-resident batches (torch tensors).  The variants of a case
run alternately, each timed --steps times after a warm-up call; the best time of each is reported, and every verdict is checked.
  one      a 1-key set (shape nb_public = 2, n_c = 1) against PlonkVerifier on the same key, 2^log2n valid proofs
  mixed16  16 keys -- the 8 pool keys of tests/golden/plonk_keys_cases.json and 8 trapdoor keys forged here -- 2^log2n shuffled proofs,
           against 16 per-key verify_batch_dev calls on the pre-sorted sub-batches (each timed alone, summed); also the PREP stage time
           of the set against the per-key contexts' PREP times summed, and of the 1-key set of `one` at the same size
  many     256 keys x 16 proofs (set-up excluded) against 256 per-key calls enqueued back to back; the 256 keys are the 8 pool keys listed
           32 times each (the set builds and reads separate tables for each, so the work is that of 256 different keys)
  setup    wall time and device memory of the set-up of 16 and of 256 keys (zkv_ctx_reserve)
Not bench.py.  PARITY UNPINNED BY CONSTRUCTION (no PLONK in the reference).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import plonk_trapdoor_keys as T                          # noqa: E402
import stylus_zkvm_verifiers_amd as zkv                  # noqa: E402

FORGED = [(1, 0), (1, 1), (3, 0), (3, 1), (8, 0), (8, 1), (31, 0), (64, 1)]


def pool():
    """The 8 pool keys in T.POOL_SHAPES order: (key bytes, proofs (4, proof bytes), inputs (4, nb_public, 32))."""
    fx = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'plonk_keys_cases.json')))
    by = {(e['nb_public'], e['n_c']): T.pool_arrays(e) for e in fx['pool']}
    return [by[sh] for sh in T.POOL_SHAPES]


def forged():
    """8 trapdoor keys and 4 valid proofs each, as pool_arrays gives them."""
    out = []
    for nb, nc in FORGED:
        rng = T.rng_for('bench-plonk-key-sets', nb, nc)
        vk = T.make_key(rng, nb, nc)
        ins = [T.inputs(('bench', nb, nc, j), nb) for j in range(4)]
        proofs = np.stack([np.frombuffer(T.forge(vk, q, rng), np.uint8) for q in ins])
        pub = np.frombuffer(b''.join(x.to_bytes(32, 'big') for q in ins for x in q), np.uint8).reshape(4, nb, 32)
        out.append((T.vk_bytes(vk), proofs, pub))
    return out


def race(fns, steps):
    """Warm-up of every variant, then `steps` rounds in which the variants run one after the other; best ms of each."""
    import torch
    for f in fns:
        f()
    torch.cuda.synchronize()
    best = [None] * len(fns)
    for _ in range(steps):
        for k, f in enumerate(fns):
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t) * 1e3
            best[k] = dt if best[k] is None or dt < best[k] else best[k]
    return best


def to_dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def rows(keys, kk, j, ps, ins):
    """Proof and input rows of the set's strides: proof j[i] of key kk[i]."""
    n = len(kk)
    proofs = np.zeros((n, ps), np.uint8)
    pub = np.zeros((n, max(ins // 32, 1), 32), np.uint8)
    for b, (_, P, Q) in enumerate(keys):
        m = kk == b
        proofs[m, :P.shape[1]] = P[j[m]]
        if Q.shape[1]:
            pub[m, :Q.shape[1]] = Q[j[m]]
    return proofs, pub


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


def tiled(key, n, seed):
    vk, P, Q = key
    j = np.random.default_rng(seed).integers(0, len(P), n)
    return P[j], Q[j]


def case_one(args, pl):
    n = 1 << args.log2n
    key = pl[T.POOL_SHAPES.index((2, 1))]
    P, Q = tiled(key, n, 1)
    s = zkv.PlonkVerifierSet([key[0]])
    v = zkv.PlonkVerifier(key[0])
    f_set, o_set = set_fn(s, np.zeros(n, np.uint32), P, Q)
    f_one, o_one = single_fn(v, P, Q)
    ms_set, ms_one = race([f_set, f_one], args.steps)
    f_set(); st_set = s.last_stage_ms()
    f_one(); st_one = v.last_stage_ms()
    assert o_set.cpu().numpy().all() and o_one.cpu().numpy().all()
    s.close(); v.close()
    return dict(case='one', n=n, set_ms=ms_set, plonk_verifier_ms=ms_one, ratio=ms_set / ms_one, set_stage_ms=st_set, single_stage_ms=st_one)


def case_mixed16(args, pl):
    n = 1 << args.log2n
    keys = pl + forged()
    K = len(keys)
    rng = np.random.default_rng(16)
    kk = rng.integers(0, K, n).astype(np.uint32)
    j = rng.integers(0, 4, n)
    s = zkv.PlonkVerifierSet([k[0] for k in keys])
    proofs, pub = rows(keys, kk, j, s.proof_stride(), s.input_stride())
    f_set, o_set = set_fn(s, kk, proofs, pub)
    vs, fns, outs, prep = [], [], [], []
    for b, key in enumerate(keys):                       # the pre-sorted sub-batches, one context per key
        m = kk == b
        v = zkv.PlonkVerifier(key[0])
        f, o = single_fn(v, key[1][j[m]], key[2][j[m]])
        vs.append(v); fns.append(f); outs.append(o)
    best = race([f_set] + fns, args.steps)
    for v, f in zip(vs, fns):
        f(); prep.append(v.last_stage_ms()[0])
    f_set(); st_set = s.last_stage_ms()
    assert o_set.cpu().numpy().all() and all(o.cpu().numpy().all() for o in outs)
    for v in vs:
        v.close()
    s.close()
    one = zkv.PlonkVerifierSet([pl[T.POOL_SHAPES.index((2, 1))][0]])
    P, Q = tiled(pl[T.POOL_SHAPES.index((2, 1))], n, 2)
    f1, o1 = set_fn(one, np.zeros(n, np.uint32), P, Q)
    race([f1], 1)
    f1(); st_one = one.last_stage_ms()
    one.close()
    return dict(case='mixed16', n=n, keys=K, set_ms=best[0], per_key_sum_ms=sum(best[1:]), ratio=best[0] / sum(best[1:]),
                set_stage_ms=st_set, set_prep_ms=st_set[0], per_key_prep_sum_ms=sum(prep), one_key_2_1_prep_ms=st_one[0],
                prep_ratio_vs_per_key=st_set[0] / sum(prep))


def case_many(args, pl):
    K, per = 256, 16
    keys = [pl[k % len(pl)] for k in range(K)]
    s = zkv.PlonkVerifierSet([k[0] for k in keys])
    s.reserve(K * per)
    kk = np.random.default_rng(1).permutation(np.repeat(np.arange(K, dtype=np.uint32), per))
    j = np.arange(K * per) % 4
    proofs, pub = rows(keys, kk, j, s.proof_stride(), s.input_stride())
    f_set, o_set = set_fn(s, kk, proofs, pub)
    vs = [zkv.PlonkVerifier(k[0]) for k in keys]
    calls = [single_fn(v, np.resize(k[1], (per, k[1].shape[1])), np.resize(k[2], (per,) + k[2].shape[1:])) for v, k in zip(vs, keys)]
    ms_set, ms_keys = race([f_set, lambda: [f() for f, _ in calls]], min(args.steps, 2))
    assert o_set.cpu().numpy().all() and all(o.cpu().numpy().all() for _, o in calls)
    for v in vs:
        v.close()
    s.close()
    return dict(case='many', keys=K, proofs_per_key=per, set_ms=ms_set, per_key_calls_ms=ms_keys, speedup=ms_keys / ms_set)


def case_setup(args, pl):
    import torch
    out = dict(case='setup')
    for K in (16, 256):
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info()
        s = zkv.PlonkVerifierSet([pl[k % len(pl)][0] for k in range(K)])
        t = time.perf_counter()
        s.reserve(1)
        s.synchronize()
        out['keys_%d_ms' % K] = (time.perf_counter() - t) * 1e3
        free1, _ = torch.cuda.mem_get_info()
        out['keys_%d_device_mb' % K] = (free0 - free1) / 2 ** 20
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='one,mixed16,many,setup')
    ap.add_argument('--log2n', type=int, default=18)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    torch.zeros(1).cuda()
    pl = pool()
    fns = dict(one=case_one, mixed16=case_mixed16, many=case_many, setup=case_setup)
    for c in args.cases.split(','):
        r = fns[c](args, pl)
        line = json.dumps(r)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
