"""Measurements of the RISC Zero router's set route (include/zkv_risc0_router_set.h).

    python tools/bench_risc0_router_set.py [--cases decode,worst,resources] [--log2n 20] [--depth 20] [--rounds 5] [--out FILE]

One JSON line per case (appended to --out, default profiles/risc0_router_set_bench.jsonl); device-resident batches (torch tensors).  The
two variants of a case alternate, one warm-up call each, then --rounds rounds; the result is the best round, every round is recorded
(HIP events around the call on its stream), every status and count is checked.
  decode     2^log2n set-inclusion seals at --depth over 16 distinct valid root seals of one keyed route (16 trees of 64 leaves whose
             paths continue over shared siblings to --depth; the claims are tiled):
             A  zkv_risc0_router_verify_ragged_dev of a router with that keyed route and the set route, on the on-chain seals;
             B  zkv_risc0_setincl_verify_batch_dev of a keyed set-inclusion context on the same claims, pre-decoded and pre-indexed
                (DESIGN section 16's case 2).
             The ratio A / B is the price of decoding the seals and finding the root seals' identity on the device.
  worst      2^14 set seals with 2^14 distinct root seals (re-randomisations of one valid root proof, so every claim is the same claim):
             A  the set router, 2^14 root jobs;
             B  zkv_risc0_router_verify_batch_dev of a router with the same keyed route and no set route, on those 2^14 root seals alone.
  resources  VGPRs, scratch and occupancy of the new kernels from the build logs -> profiles/risc0_router_set_resources.txt (no GPU needed)
Not bench.py.
"""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _alternate(torch, a, b, stream, rounds):
    """Both variants once as a warm-up, then `rounds` rounds of A, B -> ([ms of A], [ms of B])."""
    a(); b(); stream.synchronize()
    out = ([], [])
    for _ in range(rounds):
        for k, fn in enumerate((a, b)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); fn(); e1.record(stream); e1.synchronize()
            out[k].append(round(e0.elapsed_time(e1), 4))
    return out


def _summary(ms):
    return dict(best_ms=min(ms), worst_ms=max(ms), spread_ms=round(max(ms) - min(ms), 4), all_ms=ms)


def _setup(seed):
    import risc0_router_model as rm
    import spec_model as m
    rng = random.Random(seed)
    r32 = lambda: bytes(rng.randrange(256) for _ in range(32))
    key = rm.Key(seed)
    return rng, r32, key, m.sha256(b'bench_risc0_router_set %d' % seed)


class RaggedCall:
    """zkv_risc0_router_verify_ragged_dev on uploaded seals."""
    def __init__(self, torch, rt, blob, off, ids, jds, stream):
        dev = torch.device('cuda', 0)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        self.rt, self.n, self.bytes = rt, len(off) - 1, int(off[-1])
        self.t = [up(blob), up(off.astype(np.uint64).view(np.int64)), up(ids), up(jds)]
        self.st = torch.full((self.n,), 255, dtype=torch.uint8, device=dev)
        self.rv = torch.full((self.n, 4), 255, dtype=torch.uint8, device=dev)
        self.stream = stream

    def __call__(self):
        t = self.t
        self.rt.verify_ragged_dev(self.n, t[0].data_ptr(), t[1].data_ptr(), self.bytes, t[2].data_ptr(), t[3].data_ptr(), self.st.data_ptr(), self.rv.data_ptr(),
                                  self.stream.cuda_stream)


def case_decode(torch, args):
    import set_inclusion_model as sm
    import spec_model as m
    import stylus_zkvm_verifiers_amd as zkv
    rng, r32, key, set_id = _setup(0xB17)
    n, depth, trees, leaves = 1 << args.log2n, args.depth, 16, 64
    assert depth >= 6 and n % (trees * leaves) == 0
    set_sel = sm.set_selector(set_id)
    rows_id, rows_jd, rows_path, rows_idx, rows_seal, seals = [], [], [], [], [], []
    for t in range(trees):
        ids = [(r32(), r32()) for _ in range(leaves)]
        small, paths = sm.tree_paths([sm.leaf(m.receipt_claim_ok_digest(i, j)) for i, j in ids])
        upper = [r32() for _ in range(depth - 6)]
        root = small
        for s in upper:
            root = sm.node(root, s)
        seal = key.prove(set_id, sm.root_journal(set_id, root))
        seals.append(seal)
        for (i, j), p in zip(ids, paths):
            rows_id.append(i); rows_jd.append(j); rows_path.append(b''.join(p + upper)); rows_idx.append(t)
            rows_seal.append(set_sel + sm.abi_encode_seal(p + upper, seal))
    pool = len(rows_idx)
    rep = n // pool
    tile = lambda rows, w: np.tile(np.frombuffer(b''.join(rows), np.uint8).reshape(pool, w), (rep, 1)).reshape(-1)
    seal_bytes = len(rows_seal[0])
    assert all(len(s) == seal_bytes for s in rows_seal)
    stream = torch.cuda.Stream()
    rt = zkv.RiscZeroSetRouter(set_id, keyed=[key.triple()])
    ids_t, jds_t = tile(rows_id, 32), tile(rows_jd, 32)
    a = RaggedCall(torch, rt, tile(rows_seal, seal_bytes), np.arange(n + 1, dtype=np.uint64) * seal_bytes, ids_t, jds_t, stream)
    # B: the same claims pre-decoded for a keyed set-inclusion context whose inner verifier is the keyed route's
    si = zkv.RiscZeroSetInclusionVerifier(key.control_root, key.control_id, set_id, vk_words=key.words, root_selector=key.selector)
    dev = torch.device('cuda', 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    tb = [up(ids_t), up(jds_t), up(tile(rows_path, 32 * depth)), up((np.arange(n + 1, dtype=np.uint64) * depth).astype(np.uint32).view(np.int32)),
          up(np.tile(np.array(rows_idx, dtype=np.uint32), rep).view(np.int32)), up(np.frombuffer(b''.join(seals) + bytes(4), np.uint8))]
    st_b = torch.full((n,), 255, dtype=torch.uint8, device=dev); rv_b = torch.zeros((n, 4), dtype=torch.uint8, device=dev)

    def b():
        si.verify_batch_dev(n, tb[0].data_ptr(), tb[1].data_ptr(), tb[2].data_ptr(), tb[3].data_ptr(), n * depth, tb[4].data_ptr(), trees, tb[5].data_ptr(),
                            st_b.data_ptr(), rv_b.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    ms_a, ms_b = _alternate(torch, a, b, stream, args.rounds)
    ok = (not a.st.cpu().numpy().any() and not st_b.cpu().numpy().any() and rt.set_last_counts() == (n, trees, trees, 0) and si.last_counts() == (n, trees, 0))
    row = dict(case='decode', log2n=args.log2n, depth=depth, root_seals=trees, seal_bytes=seal_bytes, blob_GB=round(n * seal_bytes / 1e9, 3),
               router_ragged=_summary(ms_a), setincl_predecoded=_summary(ms_b), ratio=round(min(ms_a) / min(ms_b), 4),
               claims_per_s_router=round(n / (min(ms_a) * 1e-3)), claims_per_s_predecoded=round(n / (min(ms_b) * 1e-3)),
               setincl_stage_ms=[round(x, 3) for x in si.last_stage_ms()] if hasattr(si, 'last_stage_ms') else None, all_as_expected=bool(ok))
    rt.close(); si.close()
    return row


def case_worst(torch, args):
    import set_inclusion_model as sm
    import spec_model as m
    import stylus_zkvm_verifiers_amd as zkv
    from stylus_zkvm_verifiers_amd import synth
    rng, r32, key, set_id = _setup(0x3058)
    n, depth = 1 << 14, args.depth
    ia, jd = r32(), r32()
    path = [r32() for _ in range(depth)]
    root = sm.walk(m.receipt_claim_ok_digest(ia, jd), path)
    rj = sm.root_journal(set_id, root)
    base = key.prove(set_id, rj)
    sig = key.route.verifier.signals(m.receipt_claim_ok_digest(set_id, rj))
    proofs, _, _, _ = synth.make_groth16_batch(key.words, 'risc0', base[4:], sig, n, seed=0x3058, mutate_every=1 << 30)
    roots = np.concatenate([np.tile(np.frombuffer(key.selector, np.uint8), (n, 1)), proofs], axis=1)          # n x 260, pairwise distinct
    assert len({bytes(r) for r in roots}) == n
    head = np.frombuffer(sm.set_selector(set_id) + sm.abi_encode_seal(path, bytes(260))[:-288], np.uint8)
    seal_bytes = len(head) + 288
    blob = np.zeros((n, seal_bytes), dtype=np.uint8)
    blob[:, :len(head)] = head
    blob[:, len(head):len(head) + 260] = roots
    stream = torch.cuda.Stream()
    tile32 = lambda v: np.tile(np.frombuffer(v, np.uint8), n)
    rt = zkv.RiscZeroSetRouter(set_id, keyed=[key.triple()])
    a = RaggedCall(torch, rt, blob.reshape(-1), np.arange(n + 1, dtype=np.uint64) * seal_bytes, tile32(ia), tile32(jd), stream)
    plain = zkv.RiscZeroRouter(keyed=[key.triple()])
    plain.reserve(n)
    dev = torch.device('cuda', 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    tb = [up(roots.reshape(-1)), up(tile32(set_id)), up(tile32(rj))]
    st_b = torch.full((n,), 255, dtype=torch.uint8, device=dev)

    def b():
        plain.verify_batch_dev(n, tb[0].data_ptr(), tb[1].data_ptr(), tb[2].data_ptr(), st_b.data_ptr(), 0, stream.cuda_stream)
    torch.cuda.synchronize()
    ms_a, ms_b = _alternate(torch, a, b, stream, args.rounds)
    ok = not a.st.cpu().numpy().any() and not st_b.cpu().numpy().any() and rt.set_last_counts() == (n, n, n, 0)
    row = dict(case='worst', log2n=14, depth=depth, jobs=n, set_router=_summary(ms_a), root_seals_alone=_summary(ms_b), ratio=round(min(ms_a) / min(ms_b), 4),
               all_as_expected=bool(ok))
    rt.close(); plain.close()
    return row


def case_resources(args):
    from stylus_zkvm_verifiers_amd import build
    keep = ('VGPRs', 'AGPRs', 'TotalSGPRs', 'ScratchSize [bytes/lane]', 'Occupancy [waves/SIMD]', 'LDS Size [bytes/block]')
    rows = [r for r in build.resource_report() if 'rzset' in r['kernel']]
    path = os.path.join(ROOT, 'profiles', 'risc0_router_set_resources.txt')
    with open(path, 'w') as f:
        f.write('kernel resources of csrc/k_rzrouter_set.hip as hipcc reports them (-Rpass-analysis=kernel-resource-usage, gfx950); no existing kernel changed\n')
        for r in rows:
            f.write('%s: %s\n' % (r['kernel'], ', '.join('%s %s' % (k, r.get(k)) for k in keep)))
    return dict(case='resources', kernels=len(rows), file=os.path.relpath(path, ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='decode,worst,resources')
    ap.add_argument('--log2n', type=int, default=20)
    ap.add_argument('--depth', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'risc0_router_set_bench.jsonl'))
    args = ap.parse_args()
    cases = args.cases.split(',')
    torch = None
    if set(cases) - {'resources'}:
        import torch
    bad = False
    for c in cases:
        line = case_resources(args) if c == 'resources' else {'decode': case_decode, 'worst': case_worst}[c](torch, args)
        print(json.dumps(line), flush=True)
        with open(args.out, 'a') as f:
            f.write(json.dumps(line) + '\n')
        bad = bad or line.get('all_as_expected') is False
    if bad:
        raise SystemExit('a status or a count is not what the case expects')


if __name__ == '__main__':
    main()
