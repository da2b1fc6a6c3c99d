"""Throughput of the SP1 gateway (include/zkv_sp1_gateway.h) against the per-route contexts on pre-sorted batches.

    python tools/bench_sp1_gateway.py [--cases mixed,groth16] [--log2n-mixed 18] [--log2n-groth16 20] [--steps 5] [--out FILE]

One JSON line per case (appended to --out, default profiles/sp1_gateway_bench.jsonl); device-resident batches (torch tensors), one
warm-up call per variant, then --steps rounds in which the two variants alternate; best of the rounds.  Every status is checked
against the per-route calls.
  mixed    2^log2n-mixed proofs, 3/4 SP1 Groth16 and 1/4 SP1 PLONK in random order, through a gateway (Groth16 route + one PLONK route),
           against Sp1Verifier.verify_batch_dev + Sp1PlonkVerifier.verify_batch_dev on the same proofs sorted on the host (summed)
  groth16  2^log2n-groth16 SP1 Groth16 proofs through the same gateway against Sp1Verifier.verify_batch_dev
Proofs: the real SP1 proof re-randomised into 4,096 distinct ones (synth.make_batch), the 64-proof PLONK pool, interleaved by
synth.make_sp1_gateway_batch.  Not bench.py.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import stylus_zkvm_verifiers_amd as zkv                 # noqa: E402
from stylus_zkvm_verifiers_amd import synth             # noqa: E402

H = bytes.fromhex


def pools():
    g = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'real_proofs.json')))['sp1']
    seals, _, _, _ = synth.make_batch('sp1', H(g['proof']), 4096, 0x6A7EB, mutate_every=0)
    gp = (seals, np.tile(np.frombuffer(H(g['vkey']), np.uint8), (4096, 1)), np.tile(np.frombuffer(H(g['public_values']), np.uint8), (4096, 1)))
    pool = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'plonk_pool.json')))
    pp = tuple(np.stack([np.frombuffer(H(p[k]), np.uint8) for p in pool['proofs']]) for k in ('proof', 'vkey', 'public_values'))
    return gp, pp, (H(pool['vk']), H(pool['verifier_hash']))


def case(name, n, frac, gp, pp, key, steps):
    import torch
    dev = torch.device('cuda', 0)
    s = torch.cuda.current_stream().cuda_stream
    blob, off, vkeys, pvs, kind, _, _ = synth.make_sp1_gateway_batch(gp, pp, n, frac, 0x6A7EB + n)
    gw = zkv.Sp1Gateway(True, [key])
    refs = [zkv.Sp1Verifier(), zkv.Sp1PlonkVerifier(*key)]
    pv_len = pvs.shape[1]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev)
    d_vk, d_pv, d_p, d_off = up(vkeys), up(pvs), up(blob), up(off.view(np.int64))
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev); d_rv = torch.zeros(4 * n, dtype=torch.uint8, device=dev)
    # the per-route baseline: the same proofs, sorted on the host, fixed stride per route
    sub = []
    for k, rec in ((0, 260), (1, 868)):
        idx = np.nonzero(kind == k)[0]
        if not len(idx):
            sub.append(None)
            continue
        P = np.concatenate([blob[off[idx[c0:c0 + 8192]].astype(np.int64)[:, None] + np.arange(rec)[None, :]] for c0 in range(0, len(idx), 8192)])
        sub.append((idx, up(vkeys[idx]), up(pvs[idx]), up(P), torch.zeros(len(idx), dtype=torch.uint8, device=dev),
                    torch.zeros(4 * len(idx), dtype=torch.uint8, device=dev)))
    gw.reserve(n)
    for v in refs:
        v.reserve(n)

    def run_gw():
        gw.verify_batch_dev(n, d_vk.data_ptr(), d_pv.data_ptr(), pv_len, d_p.data_ptr(), d_off.data_ptr(), len(blob), d_st.data_ptr(), d_rv.data_ptr(), s)

    def run_ref():
        for v, x in zip(refs, sub):
            if x is not None:
                v.verify_batch_dev(len(x[0]), x[1].data_ptr(), x[2].data_ptr(), pv_len, x[3].data_ptr(), x[4].data_ptr(), x[5].data_ptr(), s)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    timed(run_gw); timed(run_ref)
    t_gw, t_ref = [], []
    for _ in range(steps):
        t_gw.append(timed(run_gw)); t_ref.append(timed(run_ref))
    st = d_st.cpu().numpy()
    want = np.zeros(n, np.uint8)
    for x in sub:
        if x is not None:
            want[x[0]] = x[4].cpu().numpy()
    ok = bool((st == want).all())
    counts = gw.last_route_counts()
    row = dict(case=name, n=n, groth16=int((kind == 0).sum()), plonk=int((kind == 1).sum()), gateway_ms=round(min(t_gw), 3),
               per_route_ms=round(min(t_ref), 3), ratio=round(min(t_gw) / min(t_ref), 4), gateway_all_ms=[round(x, 3) for x in t_gw],
               per_route_all_ms=[round(x, 3) for x in t_ref], statuses_equal=ok, accepted=int((st == 0).sum()), route_counts=counts,
               mproofs_per_s=round(n / min(t_gw) / 1e3, 3))
    gw.close()
    for v in refs:
        v.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='mixed,groth16')
    ap.add_argument('--log2n-mixed', type=int, default=18)
    ap.add_argument('--log2n-groth16', type=int, default=20)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sp1_gateway_bench.jsonl'))
    a = ap.parse_args()
    gp, pp, key = pools()
    rows = []
    for c in a.cases.split(','):
        if c == 'mixed':
            rows.append(case('mixed_3g_1p', 1 << a.log2n_mixed, 0.75, gp, pp, key, a.steps))
        elif c == 'groth16':
            rows.append(case('all_groth16', 1 << a.log2n_groth16, 1.0, gp, pp, key, a.steps))
        else:
            raise SystemExit('unknown case %r' % c)
    with open(a.out, 'a') as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + '\n')
    if not all(r['statuses_equal'] for r in rows):
        raise SystemExit('gateway statuses differ from the per-route calls')


if __name__ == '__main__':
    main()
