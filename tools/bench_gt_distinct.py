#!/usr/bin/env python3
"""Times one 2^20-proof SP1 batch whose every proof has its own random program vkey (< R) and random public values, so every lane pair
gathers its own 26 rows of the GT tables (csrc/zkv_gt.h; the bench batch repeats one set of public inputs, whose rows stay in cache).
The proofs no longer verify (they fail in the final exponentiation); only times are reported.  One process per setting:
    python tools/bench_gt_distinct.py            tables on
    ZKV_GT_WINDOW_BITS=0 python tools/bench_gt_distinct.py
Prints one JSON line: ms per step (median of --steps), the stage times of the last step, table build time and bytes."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--proofs', type=int, default=1 << 20)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--pv-bytes', type=int, default=96)
    args = ap.parse_args()
    import torch
    import stylus_zkvm_verifiers_amd as z
    from stylus_zkvm_verifiers_amd import diag_gt
    H = bytes.fromhex
    s = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'real_proofs.json')))['sp1']
    dev = torch.device('cuda', 0)
    n = args.proofs
    rng = np.random.default_rng(0x5A4B5606)
    vk = rng.integers(0, 256, (n, 32), dtype=np.uint8); vk[:, 0] &= 0x0f            # < 2^252 < R
    pv = rng.integers(0, 256, (n, args.pv_bytes), dtype=np.uint8)
    proof = np.frombuffer(H(s['proof']), np.uint8)
    d_vk, d_pv = torch.from_numpy(vk).to(dev), torch.from_numpy(pv).to(dev)
    d_proofs = torch.from_numpy(np.tile(proof, (n, 1))).to(dev)
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    v = z.Sp1Verifier(0)
    v.reserve(n)
    v.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    ms = []
    for k in range(args.steps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v.verify_batch_dev(n, d_vk.data_ptr(), d_pv.data_ptr(), pv.shape[1], d_proofs.data_ptr(), d_st.data_ptr(), 0, stream)
        torch.cuda.synchronize()
        if k:
            ms.append((time.perf_counter() - t0) * 1e3)
    info = diag_gt.info(v._h)
    print(json.dumps({'proofs': n, 'tables': info['built'], 'ms_per_step_median': float(np.median(ms)), 'ms_per_step': ms,
                      'stage_ms_last_step': [float(x) for x in v.last_stage_ms()], 'all_rejected': bool((d_st.cpu().numpy() != 0).all()),
                      'table_build_ms': info['build_ms'], 'table_bytes': info['bytes']}))
    v.close()


if __name__ == '__main__':
    main()
