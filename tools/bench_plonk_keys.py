"""Throughput of the PLONK core for any key (include/zkv_plonk_keys.h) by public-input count and commitment.

    python tools/bench_plonk_keys.py [--nb 0,2,9,128] [--nc 0,1] [--log2n 16,18] [--steps 3]

Per (nb_public, n_c, batch) one JSON line: proofs/s of device-resident batches (zkv_plonk_verify_batch_dev, best of --steps timed calls
after a warm-up call) and zkv_ctx_last_stage_ms of the last call.  Proofs: the pools of tests/golden/plonk_keys_cases.json
(trapdoor keys), tiled on the device; every proof must verify.  One more line per batch size, 'sp1_ab': the SP1 PLONK pool
(tests/golden/plonk_pool.json, the toy circuit's genuinely proved proofs) through zkv_sp1_plonk_verify_batch_dev and the same proofs
as nb_public = 2, n_c = 1 generic proofs (inputs: program vkey, hash of the public values) through zkv_plonk_verify_batch_dev, in
alternation.  Not bench.py: this is a tool of its own."""
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
H = bytes.fromhex


def timed(fn, steps):
    import torch
    fn(); torch.cuda.synchronize()
    best = None
    for _ in range(steps):
        t = time.perf_counter(); fn(); torch.cuda.synchronize(); dt = time.perf_counter() - t
        best = dt if best is None or dt < best else best
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nb', default='0,2,9,128'); ap.add_argument('--nc', default='0,1')
    ap.add_argument('--log2n', default='16,18'); ap.add_argument('--steps', type=int, default=3)
    args = ap.parse_args()
    import torch
    import stylus_zkvm_verifiers_amd as z
    from stylus_zkvm_verifiers_amd import plonk_keys
    import plonk_trapdoor_keys as T
    import spec_model as m
    fx = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'plonk_keys_cases.json')))
    for lg in [int(x) for x in args.log2n.split(',')]:
        n = 1 << lg
        for nb in [int(x) for x in args.nb.split(',')]:
            for nc in [int(x) for x in args.nc.split(',')]:
                e = next(e for e in fx['pool'] if (e['nb_public'], e['n_c']) == (nb, nc))
                vk, P, Q = T.pool_arrays(e)
                idx = np.arange(n) % len(P)
                dp = torch.from_numpy(P[idx].copy()).cuda()
                dq = torch.from_numpy(Q[idx].copy()).cuda() if nb else None
                out = torch.zeros(n, dtype=torch.uint8, device='cuda')
                v = plonk_keys.PlonkVerifier(vk)
                v.reserve(n)
                best = timed(lambda: v.verify_batch_dev(n, dp.data_ptr(), dq.data_ptr() if nb else 0, out.data_ptr()), args.steps)
                assert int(out.sum()) == n, 'a pool proof failed'
                print(json.dumps(dict(bench='plonk_keys', nb_public=nb, n_c=nc, log2n=lg, proofs_per_s=round(n / best),
                                      ms=round(best * 1e3, 2), stage_ms=[round(x, 2) for x in v.last_stage_ms()])), flush=True)
                v.close()
                del dp, dq, out
        # A/B on the same proofs: SP1 PLONK context against the generic context with the same key
        pool = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'plonk_pool.json')))
        ps = pool['proofs']
        k = len(ps)
        idx = np.arange(n) % k
        sp1_proofs = np.stack([np.frombuffer(H(p['proof']), np.uint8) for p in ps])[idx]
        vkeys = np.stack([np.frombuffer(H(p['vkey']), np.uint8) for p in ps])[idx]
        pv = [H(p['public_values']) for p in ps]
        assert len({len(x) for x in pv}) == 1
        pvs = np.stack([np.frombuffer(x, np.uint8) for x in pv])[idx]
        hashes = np.stack([np.frombuffer(m.be32(m.sp1_hash_public_values(x)), np.uint8) for x in pv])[idx]
        gen_pub = np.stack([vkeys, hashes], axis=1)
        d_sp = torch.from_numpy(np.ascontiguousarray(sp1_proofs)).cuda()
        d_gp = torch.from_numpy(np.ascontiguousarray(sp1_proofs[:, 4:])).cuda()
        d_vk = torch.from_numpy(np.ascontiguousarray(vkeys)).cuda()
        d_pv = torch.from_numpy(np.ascontiguousarray(pvs)).cuda()
        d_gi = torch.from_numpy(np.ascontiguousarray(gen_pub)).cuda()
        st = torch.zeros(n, dtype=torch.uint8, device='cuda')
        ok = torch.zeros(n, dtype=torch.uint8, device='cuda')
        sp = z.Sp1PlonkVerifier(H(pool['vk']), H(pool['verifier_hash']))
        gv = plonk_keys.PlonkVerifier(H(pool['vk']))
        sp.reserve(n); gv.reserve(n)
        L = sp._L
        run_sp = lambda: L.zkv_sp1_plonk_verify_batch_dev(sp._h, n, d_vk.data_ptr(), d_pv.data_ptr(), len(pv[0]), d_sp.data_ptr(), st.data_ptr(), None, None)
        run_g = lambda: gv.verify_batch_dev(n, d_gp.data_ptr(), d_gi.data_ptr(), ok.data_ptr())
        t_sp, t_g = [], []
        for _ in range(args.steps):
            t_sp.append(timed(run_sp, 1)); t_g.append(timed(run_g, 1))
        assert int((st == 0).sum()) == n and int(ok.sum()) == n, 'a pool proof failed'
        print(json.dumps(dict(bench='plonk_keys', sp1_ab=True, nb_public=2, n_c=1, log2n=lg, sp1_plonk_proofs_per_s=round(n / min(t_sp)),
                              generic_proofs_per_s=round(n / min(t_g)), sp1_ms=round(min(t_sp) * 1e3, 2), generic_ms=round(min(t_g) * 1e3, 2))), flush=True)
        sp.close(); gv.close()


if __name__ == '__main__':
    main()
