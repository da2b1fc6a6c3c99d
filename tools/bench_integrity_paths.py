"""verify_integrity against verify on the device-resident paths (include/zkv.h: zkv_risc0_verify_integrity_batch_dev, and the mixed
call with a per-proof method, zkv_mixed_verify_call_batch_dev).

    python tools/bench_integrity_paths.py [--log2n 16,20] [--mixed-log2n 19] [--steps 5]

One JSON line per measurement, everything resident in HBM on device 0:
  - single context: verify_batch_dev and verify_integrity_batch_dev on the same 2^k seals (4,096 distinct re-randomisations of the real
    RISC Zero proof, tiled on the device), timed in alternation, best of --steps calls after a warm-up call of each;
  - mixed: 2^k proofs, a third each RISC Zero verify, RISC Zero verify_integrity and SP1 (seeded), against the same proofs with every
    RISC Zero row a verify call through zkv_mixed_verify_batch_dev (the all-verify mixed batch).
Every proof is valid and every status is checked to be 0.  Not bench.py: a tool of its own.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H = bytes.fromhex


def timed(fn, sync):
    sync()
    t = time.perf_counter()
    fn()
    sync()
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--log2n', default='16,20')
    ap.add_argument('--mixed-log2n', default='19')
    ap.add_argument('--steps', type=int, default=5)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1')
    import numpy as np
    import torch
    import stylus_zkvm_verifiers_amd as z
    from stylus_zkvm_verifiers_amd import synth
    g = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'real_proofs.json')))
    r, s = g['risc0'], g['sp1']
    dev = torch.device('cuda', 0)
    sync = torch.cuda.synchronize
    K = 4096
    seals0, _, _, _ = synth.make_batch('risc0', H(r['seal']), K, 0x1A7EB001, pool=16, mutate_every=0)
    seals1, _, _, _ = synth.make_batch('sp1', H(s['proof']), K, 0x1A7EB002, pool=16, mutate_every=0)
    row = lambda h, k: torch.from_numpy(np.tile(np.frombuffer(H(h), dtype=np.uint8), (k, 1))).to(dev)
    d0 = torch.from_numpy(seals0).to(dev)
    d1 = torch.from_numpy(seals1).to(dev)
    v = z.RiscZeroVerifier()
    v.initialize(H(r['control_root']), H(r['bn254_control_id']))
    out = []
    for lg in [int(x) for x in args.log2n.split(',') if x]:
        n = 1 << lg
        seals = d0.repeat((n + K - 1) // K, 1)[:n].contiguous()
        ids, jds, cds = row(r['image_id'], n), row(r['journal_digest'], n), row(r['claim_digest'], n)
        st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
        v.reserve(n)
        call = {'verify': lambda: v.verify_batch_dev(n, seals.data_ptr(), ids.data_ptr(), jds.data_ptr(), st.data_ptr()),
                'verify_integrity': lambda: v.verify_integrity_batch_dev(n, seals.data_ptr(), cds.data_ptr(), st.data_ptr())}
        best = {}
        for name in call:                                                # warm-up, and every status checked
            st.fill_(255); timed(call[name], sync)
            assert int((st != 0).sum()) == 0, name
        for _ in range(args.steps):
            for name in call:
                t = timed(call[name], sync)
                best[name] = min(best.get(name, t), t)
        for name in call:
            rec = {'what': 'risc0_dev', 'call': name, 'n': n, 'best_ms': round(best[name] * 1e3, 3), 'proofs_per_s': round(n / best[name]),
                   'steps': args.steps}
            out.append(rec); print(json.dumps(rec), flush=True)
        rec = {'what': 'risc0_dev_ratio', 'n': n, 'integrity_over_verify': round(best['verify_integrity'] / best['verify'], 4)}
        out.append(rec); print(json.dumps(rec), flush=True)
        del seals, ids, jds, cds, st
    mx = z.MixedVerifier(H(r['control_root']), H(r['bn254_control_id']))
    pvl = len(H(s['public_values']))
    for lg in [int(x) for x in args.mixed_log2n.split(',') if x]:
        n = 1 << lg
        rng = np.random.default_rng(0x1A7EB003)
        kind = rng.integers(0, 3, n)                                     # 0 verify, 1 verify_integrity, 2 SP1
        vm = torch.from_numpy((kind == 2).astype(np.uint8)).to(dev)
        method = torch.from_numpy((kind == 1).astype(np.uint8)).to(dev)
        pick = torch.from_numpy(rng.integers(0, K, n)).to(dev)
        sp1 = torch.from_numpy(kind == 2).to(dev).reshape(-1, 1)
        integ = torch.from_numpy(kind == 1).to(dev).reshape(-1, 1)
        seals = torch.where(sp1, d1[pick], d0[pick]).contiguous()
        a_v = torch.where(sp1, row(s['vkey'], n), row(r['image_id'], n)).contiguous()          # all-verify batch
        a_c = torch.where(integ, row(r['claim_digest'], n), a_v).contiguous()                  # a third verify_integrity
        b = torch.zeros((n, max(32, pvl)), dtype=torch.uint8, device=dev)
        b[:, :pvl] = torch.where(sp1, row(s['public_values'], n), torch.zeros((n, pvl), dtype=torch.uint8, device=dev))
        b[:, :32] = torch.where(sp1, b[:, :32], row(r['journal_digest'], n))
        b = b.contiguous()
        st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
        mx.reserve(n)
        call = {'all_verify': lambda: mx.verify_batch_dev(n, vm.data_ptr(), seals.data_ptr(), a_v.data_ptr(), b.data_ptr(), b.shape[1], pvl, st.data_ptr()),
                'third_integrity': lambda: mx.verify_batch_dev(n, vm.data_ptr(), seals.data_ptr(), a_c.data_ptr(), b.data_ptr(), b.shape[1], pvl, st.data_ptr(),
                                                               d_method=method.data_ptr())}
        best = {}
        for name in call:
            st.fill_(255); timed(call[name], sync)
            assert int((st != 0).sum()) == 0, name
        for _ in range(args.steps):
            for name in call:
                t = timed(call[name], sync)
                best[name] = min(best.get(name, t), t)
        for name in call:
            rec = {'what': 'mixed_dev', 'batch': name, 'n': n, 'best_ms': round(best[name] * 1e3, 3), 'proofs_per_s': round(n / best[name]),
                   'steps': args.steps, 'rows': {'verify': int((kind == 0).sum()), 'verify_integrity': int((kind == 1).sum()) if name == 'third_integrity' else 0,
                                                 'sp1': int((kind == 2).sum())}}
            out.append(rec); print(json.dumps(rec), flush=True)
        rec = {'what': 'mixed_dev_ratio', 'n': n, 'third_integrity_over_all_verify': round(best['third_integrity'] / best['all_verify'], 4)}
        out.append(rec); print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
