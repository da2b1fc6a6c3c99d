"""Cost of the calldata front end of deployed Groth16 key sets (include/zkv_groth16_set_wire.h):
zkv_groth16_set_eth_call_batch_dev on raw verifyProof calldata against zkv_groth16_set_verify_batch_dev on the same batch, decoded
beforehand -- the existing call is the yardstick, not the code under test.

    python tools/bench_groth16_set_wire.py [--cases mixed16,long129] [--steps 5] [--out profiles/groth16_set_wire_ab.txt] [--dry]

  mixed16  2^18 requests over 16 contracts, n_ic in {2, 3, 5, 7, 9, 17}, both forms and both conventions, shuffled
  long129  2^16 requests to one 129-IC contract
The two calls alternate, --steps times after a warm-up of each; per call the best and the median host time around a device
synchronisation, the decode kernel's event time (zkv_ctx_last_wire_ms) and the bytes it reads and writes, computed from the shapes.
Every status is compared with the decoded call's verdict.  --dry builds the batches and stops before the device.  Not bench.py.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

import spec_model as m                                  # noqa: E402
import stylus_zkvm_verifiers_amd as zkv                 # noqa: E402
from stylus_zkvm_verifiers_amd import build, synth      # noqa: E402
from stylus_zkvm_verifiers_amd import groth16_set_wire as gw   # noqa: E402

VM = {'risc0': 0, 'sp1': 1}
POOL = 4096                                             # distinct proofs per key, tiled


def key_batch(rng, n_ic, vm, seed):
    vk, td = m.trapdoor_vk(rng, n_ic)
    sig = [rng.randrange(m.R) for _ in range(n_ic - 1)]
    base = m.proof_to_words(*m.trapdoor_prove(rng, td, sig, vm))
    vkb = m.vk_to_words(vk)
    # one proof in 64 is damaged; none by a signal >= r, which the wire call would not place: both calls verify the same proofs
    classes = [c for c in synth.GROTH16_MUTATION_CLASSES if c != 'signal_eq_r']
    p, s, _, _ = synth.make_groth16_batch(vkb, vm, base, sig, POOL, seed=seed, mutate_every=64, classes=classes)
    return (vkb, n_ic, VM[vm]), p, s


def make_case(n_ics, n, seed):
    """-> keys for Groth16DeployedSet, and the batch both ways: (to, blob, offsets) and (key, proofs, signal rows)."""
    rng = random.Random(seed)
    K, per = len(n_ics), n // len(n_ics)
    stride = max(n_ics) - 1
    keys, kk, proofs = [], np.repeat(np.arange(K, dtype=np.uint32), per), np.zeros((n, 256), np.uint8)
    sigs = np.zeros((n, stride, 32), np.uint8)
    for j, n_ic in enumerate(n_ics):
        key, p, s = key_batch(rng, n_ic, 'risc0' if j % 2 else 'sp1', seed + j)
        keys.append(key + (bytes(rng.randrange(256) for _ in range(20)), (j // 2) % 2))
        idx = np.arange(per) % POOL
        proofs[per * j:per * (j + 1)] = p[idx]
        sigs[per * j:per * (j + 1), :n_ic - 1] = s[idx]
    perm = np.random.default_rng(seed).permutation(n)
    kk, proofs, sigs = kk[perm], proofs[perm], sigs[perm]
    lens = np.array([4 + 32 * (8 + k[1] - 1) for k in keys], dtype=np.uint64)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens[kk])
    blob = np.zeros(int(off[n]), np.uint8)
    to = np.frombuffer(b''.join(k[3] for k in keys), np.uint8).reshape(K, 20)[kk]
    for j, k in enumerate(keys):
        L, sel = int(lens[j]), np.frombuffer(gw.selector(k[4], k[1] - 1), np.uint8)
        rows = np.nonzero(kk == j)[0]
        for c in range(0, len(rows), 4096):              # (bounded index arrays)
            r = rows[c:c + 4096]
            body = np.concatenate([np.broadcast_to(sel, (len(r), 4)), proofs[r], sigs[r, :k[1] - 1].reshape(len(r), -1)], axis=1)
            blob[(off[r].astype(np.int64)[:, None] + np.arange(L)[None, :]).ravel()] = body.ravel()
    return keys, (np.ascontiguousarray(to), blob, off), (kk, proofs, sigs)


def run_case(name, n_ics, n, steps, dry):
    import torch
    keys, (to, blob, off), (kk, proofs, sigs) = make_case(n_ics, n, 1 + len(n_ics))
    i = n // 3                                           # the blob holds what the encoder gives
    assert blob[int(off[i]):int(off[i + 1])].tobytes() == gw.encode_call(keys[kk[i]][4], proofs[i].tobytes(), [s.tobytes() for s in sigs[i, :keys[kk[i]][1] - 1]])
    n_sig = np.array([k[1] - 1 for k in keys])[kk]
    read = 20 * n + 8 * (n + 1) + len(blob)
    written = int((256 + 32 * n_sig + 10).sum())
    res = dict(case=name, n=n, keys=len(keys), calldata_bytes=len(blob), decode_bytes_read=read, decode_bytes_written=written)
    if dry:
        return res
    dev = torch.device('cuda', 0)
    s = zkv.Groth16DeployedSet(keys)
    s.reserve(n)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_to, d_cd, d_off = T(to), T(blob), T(off.astype(np.int64))
    d_k, d_p, d_s = T(kk.view(np.int32)), T(proofs), T(sigs.reshape(n, -1))
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev); d_v = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    wire = lambda: s.eth_call_batch_dev(n, d_to.data_ptr(), d_cd.data_ptr(), d_off.data_ptr(), len(blob), d_st.data_ptr())
    decoded = lambda: s.verify_batch_dev(n, d_k.data_ptr(), d_p.data_ptr(), d_s.data_ptr(), d_v.data_ptr())
    for fn in (wire, decoded):
        fn(); torch.cuda.synchronize()
    st, v = d_st.cpu().numpy(), d_v.cpu().numpy()
    assert set(np.unique(st)) <= {0, 1} and ((st == 0) == (v == 1)).all() and 0 < (st == 1).mean() < 0.1
    assert s.last_call_counts() == [n, 0, 0, 0]
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
               decode_kernel_ms=k_ms, decode_kernel_share_of_call=k_ms / statistics.median(t_wire),
               decode_read_GBps=read / k_ms / 1e6, decode_read_plus_written_GBps=(read + written) / k_ms / 1e6,
               rejected_fraction=float((st == 1).mean()), stage_ms=s.last_stage_ms())
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='mixed16,long129')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--log2n', type=int, default=0, help='override both sizes (rehearsals)')
    ap.add_argument('--out', default='')
    ap.add_argument('--dry', action='store_true')
    args = ap.parse_args()
    cases = dict(mixed16=([(2, 3, 5, 7, 9, 17)[j % 6] for j in range(16)], 1 << (args.log2n or 18)), long129=([129], 1 << (args.log2n or 16)))
    lines = []
    for c in args.cases.split(','):
        lines.append(json.dumps(run_case(c, cases[c][0], cases[c][1], args.steps, args.dry)))
        print(lines[-1], flush=True)
    for r in build.resource_report():
        if 'k_gset_wire' in r['kernel']:
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
