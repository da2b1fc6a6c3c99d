"""Throughput of Groth16 key sets (include/zkv_groth16_set.h) against per-key Groth16Verifier contexts.

    python tools/bench_groth16_key_sets.py [--cases one,mixed16,many,setup] [--log2n 18] [--steps 3]

One JSON line per case; device-resident batches (torch tensors), best of --steps timed calls after a warm-up call, every proof checked.
  one      a 1-key set (n_ic = 3) against Groth16Verifier on the same key with ZKV_LONG_KEY=1 (the same vk_x walk), 2^log2n proofs
  mixed16  16 keys, n_ic in {2, 3, 5, 7, 9, 17}, 2^log2n shuffled proofs, against 16 per-key verify_batch_dev calls on the pre-sorted
           sub-batches (summed)
  many     1,024 keys x 16 proofs (set-up excluded) against 1,024 per-key calls; the 1,024 keys are one trapdoor key listed 1,024 times
           (the set builds and reads separate tables for each, so the work is that of 1,024 different keys)
  setup    wall time of the set-up of 1,024 keys with n_ic = 3 (zkv_ctx_reserve), and of 64 keys for comparison
Proofs: one trapdoor proof per key re-randomised into 4,096 distinct ones (synth.make_groth16_batch), tiled.  Not bench.py.
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

import spec_model as m                                  # noqa: E402
import stylus_zkvm_verifiers_amd as zkv                 # noqa: E402
from stylus_zkvm_verifiers_amd import synth             # noqa: E402

VM = {'risc0': 0, 'sp1': 1}


def key_batch(rng, n_ic, vm, count, seed):
    vk, td = m.trapdoor_vk(rng, n_ic)
    sig = [rng.randrange(m.R) for _ in range(n_ic - 1)]
    base = m.proof_to_words(*m.trapdoor_prove(rng, td, sig, vm))
    vkb = m.vk_to_words(vk)
    p, s, _, _ = synth.make_groth16_batch(vkb, vm, base, sig, count, seed=seed, mutate_every=1 << 30)
    return (vkb, n_ic, VM[vm]), p, s


def timed(fn, steps):
    import torch
    fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(steps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t) * 1e3
        best = dt if best is None or dt < best else best
    return best


def to_dev(*arrays):
    import torch
    dev = torch.device('cuda', 0)
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def set_call(s, kk, p, sg, steps):
    import torch
    n = len(kk)
    d_k, d_p, d_s = to_dev(kk.view(np.int32), p, sg.reshape(n, -1) if sg.size else np.zeros((n, 1), np.uint8))
    d_v = torch.zeros(n, dtype=torch.uint8, device=d_p.device)
    ms = timed(lambda: s.verify_batch_dev(n, d_k.data_ptr(), d_p.data_ptr(), d_s.data_ptr(), d_v.data_ptr()), steps)
    return ms, d_v.cpu().numpy()


def single_call(v, p, sg, steps):
    import torch
    n = len(p)
    d_p, d_s = to_dev(p, sg.reshape(n, -1) if sg.size else np.zeros((n, 1), np.uint8))
    d_v = torch.zeros(n, dtype=torch.uint8, device=d_p.device)
    fn = lambda: v.verify_batch_dev(n, d_p.data_ptr(), d_s.data_ptr() if sg.size else 0, d_v.data_ptr())
    return fn, d_v


def case_one(args):
    rng = random.Random(1)
    n = 1 << args.log2n
    key, p, sg = key_batch(rng, 3, 'sp1', 4096, 1)
    p, sg = np.tile(p, (n // 4096, 1)), np.tile(sg, (n // 4096, 1, 1))
    s = zkv.Groth16VerifierSet([key])
    ms_set, out = set_call(s, np.zeros(n, np.uint32), p, sg, args.steps)
    assert out.all()
    os.environ['ZKV_LONG_KEY'] = '1'
    v = zkv.Groth16Verifier(*key)
    del os.environ['ZKV_LONG_KEY']
    fn, d_v = single_call(v, p, sg, args.steps)
    ms_one = timed(fn, args.steps)
    assert d_v.cpu().numpy().all()
    return dict(case='one', n=n, set_ms=ms_set, single_long_key_ms=ms_one, ratio=ms_set / ms_one, set_stage_ms=s.last_stage_ms())


def case_mixed16(args):
    rng = random.Random(16)
    n = 1 << args.log2n
    per = n // 16
    keys, ps, ss = [], [], []
    for j in range(16):
        key, p, sg = key_batch(rng, (2, 3, 5, 7, 9, 17)[j % 6], 'risc0' if j % 2 else 'sp1', 4096, 100 + j)
        keys.append(key); ps.append(np.tile(p, (per // 4096, 1))); ss.append(np.tile(sg, (per // 4096, 1, 1)))
    total = 0.0
    for key, p, sg in zip(keys, ps, ss):
        v = zkv.Groth16Verifier(*key)
        fn, d_v = single_call(v, p, sg, args.steps)
        total += timed(fn, args.steps)
        assert d_v.cpu().numpy().all()
        v.close()
    kk = np.repeat(np.arange(16, dtype=np.uint32), per)
    sigs = np.zeros((n, 16, 32), np.uint8)
    for j, sg in enumerate(ss):
        sigs[per * j:per * (j + 1), :sg.shape[1]] = sg
    perm = np.random.default_rng(0).permutation(n)
    s = zkv.Groth16VerifierSet(keys)
    ms_set, out = set_call(s, kk[perm], np.concatenate(ps)[perm], sigs[perm], args.steps)
    assert out.all()
    return dict(case='mixed16', n=n, set_ms=ms_set, per_key_sum_ms=total, ratio=ms_set / total, set_stage_ms=s.last_stage_ms())


def case_many(args):
    rng = random.Random(1024)
    key, p, sg = key_batch(rng, 3, 'sp1', 4096, 7)
    K, per = 1024, 16
    s = zkv.Groth16VerifierSet([key] * K)
    s.reserve(K * per)
    kk = np.random.default_rng(1).permutation(np.repeat(np.arange(K, dtype=np.uint32), per))
    idx = np.arange(K * per) % 4096
    ms_set, out = set_call(s, kk, p[idx], sg[idx], args.steps)
    assert out.all()
    s.close()
    os.environ['ZKV_LONG_KEY'] = '1'                     # (no 16-bit window rows: 1,024 contexts of those would not fit)
    vs = [zkv.Groth16Verifier(*key) for _ in range(K)]
    del os.environ['ZKV_LONG_KEY']
    calls = [single_call(v, p[:per], sg[:per], 1) for v in vs]
    for fn, _ in calls:
        fn()
    import torch
    torch.cuda.synchronize()
    ms_keys = timed(lambda: [fn() for fn, _ in calls], min(args.steps, 2))
    assert all(d.cpu().numpy().all() for _, d in calls)
    for v in vs:
        v.close()
    return dict(case='many', keys=K, proofs_per_key=per, set_ms=ms_set, per_key_calls_ms=ms_keys, speedup=ms_keys / ms_set)


def case_setup(args):
    rng = random.Random(3)
    vk, _ = m.trapdoor_vk(rng, 3)
    key = (m.vk_to_words(vk), 3, 1)
    out = []
    for K in (64, 1024):
        s = zkv.Groth16VerifierSet([key] * K)
        t = time.perf_counter()
        s.reserve(1)
        out.append(dict(keys=K, setup_ms=(time.perf_counter() - t) * 1e3))
        s.close()
    return dict(case='setup', n_ic=3, runs=out, setup_launches=6, note='six set-up kernels whatever the key count (k_gset.hip launch_gset_setup)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='one,mixed16,many,setup')
    ap.add_argument('--log2n', type=int, default=18)
    ap.add_argument('--steps', type=int, default=3)
    args = ap.parse_args()
    fns = dict(one=case_one, mixed16=case_mixed16, many=case_many, setup=case_setup)
    for c in args.cases.split(','):
        print(json.dumps(fns[c](args)), flush=True)


if __name__ == '__main__':
    main()
