"""Cost of the calldata front end of deployed PLONK key sets (include/zkv_plonk_set_wire.h):
zkv_plonk_set_eth_call_batch_dev on raw Verify(bytes,uint256[]) calldata against zkv_plonk_set_verify_batch_dev on the same batch, decoded
beforehand -- the existing call is the yardstick, not the code under test.

    python tools/bench_plonk_set_wire.py [--cases mixed16,long128] [--steps 5] [--out profiles/plonk_set_wire_ab.txt] [--dry]

  mixed16  2^18 requests over 16 contracts: six pool keys of tests/golden/plonk_keys_cases.json (nb in {0, 2, 9}, both n_c), each at two
           or three addresses, shuffled
  long128  2^16 requests to one contract with 128 inputs and a commitment
One request in 64 is damaged at the pairing (the low bit of l(zeta)), so every request is placed and both calls verify the same proofs.
The two calls alternate, --steps times after a warm-up of each; per call the best and the median host time around a device
synchronisation, the event time of the decode and point kernels together (zkv_ctx_last_wire_ms) and the bytes the decode reads and
writes, computed from the shapes.  Every status is compared with the decoded call's verdict.  --dry builds the batches and stops before
the device.  Not bench.py.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import plonk_trapdoor_keys as T                         # noqa: E402
import stylus_zkvm_verifiers_amd as zkv                 # noqa: E402
from stylus_zkvm_verifiers_amd import build             # noqa: E402
from stylus_zkvm_verifiers_amd import plonk_set_wire as pw   # noqa: E402


def make_case(shapes, n, seed):
    """shapes: (nb, n_c) per contract, pool shapes.  -> keys for PlonkDeployedSet, and the batch both ways: (to, blob, offsets) and (key,
    proof rows, input rows)."""
    fx = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'plonk_keys_cases.json')))
    pool = {(e['nb_public'], e['n_c']): T.pool_arrays(e) for e in fx['pool']}
    K, per = len(shapes), n // len(shapes)
    ps, nb_max = 32 * (24 + 3 * max(nc for _, nc in shapes)), max(nb for nb, _ in shapes)
    rng = np.random.default_rng(seed)
    keys, kk = [], np.repeat(np.arange(K, dtype=np.uint32), per)
    proofs, pub = np.zeros((n, ps), np.uint8), np.zeros((n, max(nb_max, 1), 32), np.uint8)
    for j, sh in enumerate(shapes):
        vk, P, Q = pool[sh]
        keys.append((vk, hashlib.sha256(b'bench contract %d' % j).digest()[:20]))
        idx = rng.integers(0, len(P), per)
        proofs[per * j:per * (j + 1), :P.shape[1]] = P[idx]
        if sh[0]:
            pub[per * j:per * (j + 1), :sh[0]] = Q[idx]
    perm = rng.permutation(n)
    kk, proofs, pub = kk[perm], proofs[perm], pub[perm]
    proofs[np.arange(63, n, 64), 12 * 32 + 31] ^= 1     # one request in 64 fails at the pairing
    lens = np.array([4 + 96 + 32 * (24 + 3 * nc) + 32 + 32 * nb for nb, nc in shapes], dtype=np.uint64)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens[kk])
    blob = np.zeros(int(off[n]), np.uint8)
    to = np.frombuffer(b''.join(k[1] for k in keys), np.uint8).reshape(K, 20)[kk]
    word = lambda v: np.frombuffer(int(v).to_bytes(32, 'big'), np.uint8)
    for j, (nb, nc) in enumerate(shapes):
        L, lp = int(lens[j]), 32 * (24 + 3 * nc)
        head = np.concatenate([np.frombuffer(pw.selector(), np.uint8), word(0x40), word(0x60 + lp), word(lp)])
        rows = np.nonzero(kk == j)[0]
        for c in range(0, len(rows), 4096):              # (bounded index arrays)
            r = rows[c:c + 4096]
            body = np.concatenate([np.broadcast_to(head, (len(r), 100)), proofs[r, :lp], np.broadcast_to(word(nb), (len(r), 32)),
                                   pub[r, :nb].reshape(len(r), -1)], axis=1)
            blob[(off[r].astype(np.int64)[:, None] + np.arange(L)[None, :]).ravel()] = body.ravel()
    return keys, shapes, (np.ascontiguousarray(to), blob, off), (kk, proofs, pub[:, :nb_max])


def run_case(name, shapes, n, steps, dry):
    keys, shapes, (to, blob, off), (kk, proofs, pub) = make_case(shapes, n, 1 + len(shapes))
    i = n // 3                                           # the blob holds what the encoder gives
    nb, nc = shapes[kk[i]]
    assert blob[int(off[i]):int(off[i + 1])].tobytes() == pw.encode_call(proofs[i, :32 * (24 + 3 * nc)].tobytes(), [w.tobytes() for w in pub[i, :nb]])
    nbs, ncs = np.array([s[0] for s in shapes])[kk], np.array([s[1] for s in shapes])[kk]
    read = 20 * n + 8 * (n + 1) + len(blob)
    written = int((proofs.shape[1] + 32 * nbs + 12).sum())
    res = dict(case=name, n=n, contracts=len(keys), calldata_bytes=len(blob), decode_bytes_read=read, decode_bytes_written=written,
               points_tested=int((9 + ncs).sum()))
    if dry:
        return res
    import torch
    dev = torch.device('cuda', 0)
    s = zkv.PlonkDeployedSet(keys)
    s.reserve(n)
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_to, d_cd, d_off = D(to), D(blob), D(off.astype(np.int64))
    d_k, d_p = D(kk.view(np.int32)), D(proofs)
    d_i = D(pub.reshape(n, -1)) if pub.shape[1] else None
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev); d_v = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    wire = lambda: s.eth_call_batch_dev(n, d_to.data_ptr(), d_cd.data_ptr(), d_off.data_ptr(), len(blob), d_st.data_ptr())
    decoded = lambda: s.verify_batch_dev(n, d_k.data_ptr(), d_p.data_ptr(), d_i.data_ptr() if d_i is not None else 0, d_v.data_ptr())
    for fn in (wire, decoded):
        fn(); torch.cuda.synchronize()
    st, v = d_st.cpu().numpy(), d_v.cpu().numpy()
    assert set(np.unique(st)) <= {0, 1} and ((st == 0) == (v == 1)).all() and 0 < (st == 1).mean() < 0.1
    assert s.last_call_counts() == [n, 0, 0, 0, 0, 0, 0, 0]
    t_wire, t_dec, t_kernel = [], [], []
    for _ in range(steps):
        for fn, acc in ((wire, t_wire), (decoded, t_dec)):
            t = time.perf_counter()
            fn(); torch.cuda.synchronize()
            acc.append((time.perf_counter() - t) * 1e3)
        t_kernel.append(s.last_wire_ms())
    k_ms = statistics.median(t_kernel)
    res.update(wire_ms_best=min(t_wire), wire_ms_median=statistics.median(t_wire), decoded_ms_best=min(t_dec), decoded_ms_median=statistics.median(t_dec),
               ratio_best=min(t_wire) / min(t_dec), ratio_median=statistics.median(t_wire) / statistics.median(t_dec),
               decode_and_points_ms=k_ms, decode_and_points_share_of_call=k_ms / statistics.median(t_wire),
               read_GBps=read / k_ms / 1e6, read_plus_written_GBps=(read + written) / k_ms / 1e6,
               rejected_fraction=float((st == 1).mean()), stage_ms=s.last_stage_ms())
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='mixed16,long128')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--log2n', type=int, default=0, help='override both sizes (rehearsals)')
    ap.add_argument('--out', default='')
    ap.add_argument('--dry', action='store_true')
    args = ap.parse_args()
    cases = dict(mixed16=([T.POOL_SHAPES[j % 6] for j in range(16)], 1 << (args.log2n or 18)), long128=([(128, 1)], 1 << (args.log2n or 16)))
    lines = []
    for c in args.cases.split(','):
        lines.append(json.dumps(run_case(c, cases[c][0], cases[c][1], args.steps, args.dry)))
        print(lines[-1], flush=True)
    for r in build.resource_report():
        if 'k_pset_wire' in r['kernel']:
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
