"""Measurements of the RISC Zero set-inclusion path (include/zkv_risc0_set_inclusion.h).

    python tools/bench_set_inclusion.py [--cases hash,honest,worst,resources] [--log2n 20] [--depth 20] [--steps 5] [--out FILE]

One JSON line per case (appended to --out, default profiles/set_inclusion_bench.jsonl); device-resident batches (torch tensors), best of
--steps timed calls after a warm-up call (HIP events around the call on its stream; k_setincl_hash from zkv_ctx_last_stage_ms[0]).
  hash       2^log2n claims at --depth in stored-root mode (no root job runs): the call and the hash kernel, the kernel as a fraction of
             the VALU issue roofs measured in the same run (zkv_diag_issue_rate: v_mad_u64_u32 as in DESIGN section 3, and v_add_u32) and
             against the bytes it reads
  honest     the same number of claims over 16 root seals of a trapdoor key (16 trees of 64 leaves whose paths continue over shared
             siblings to --depth; the claims are tiled), against zkv_groth16_verify_batch_dev on those 16 proofs alone
  worst      2^14 claims with random paths under ONE seal -- every claim a straggler, 2^14 root jobs --, against the inner device call
             on 2^14 proofs
  resources  VGPRs, scratch and occupancy of the new kernels from the build logs -> profiles/set_inclusion_resources.txt (no GPU needed)
Set ZKV_LIB_PATH to measure another build of the library (tools/ab_build.py, e.g. -DZKV_KECCAK_UNROLL=2).  Not bench.py.
"""
import argparse
import ctypes as C
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

STORED = 0xFFFFFFFF
# VALU instructions the compiler emits (hipcc -S of csrc/k_setincl.hip for gfx950): one round of keccak-f is 120 v_bitop3_b32, 58
# v_alignbit_b32, 2 v_xor_b32 and 8 v_mov_b32; one SHA-256 compression about 1,580 (the four of the claim chain: 6,320)
VALU_PER_ROUND, VALU_PER_SHA = 188, 1580


def _events(torch, fn, stream, steps):
    fn(); stream.synchronize()
    best = None
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream); fn(); b.record(stream); b.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None else min(best, ms)
    return best


def _stage_ms(v):
    from stylus_zkvm_verifiers_amd import _lib
    out = (C.c_float * 5)()
    _lib.check(_lib.lib().zkv_ctx_last_stage_ms(v.handle, out), 'zkv_ctx_last_stage_ms')
    return [float(x) for x in out]


def _issue_roofs(device=0):
    from stylus_zkvm_verifiers_amd import _lib
    L = _lib.lib()
    roofs = {}
    for name, kind in (('v_mad_u64_u32', 0), ('v_add_u32', 2)):
        best = 0.0
        for w in (2, 4, 8):
            r = C.c_double(0)
            _lib.check(L.zkv_diag_issue_rate(device, kind, w, 2000, C.byref(r), None), 'zkv_diag_issue_rate')
            best = max(best, r.value)
        roofs[name] = best
    return roofs


def _trapdoor(seed):
    import set_inclusion_model as sm
    import spec_model as m
    rng = random.Random(seed)
    r32 = lambda: bytes(rng.randrange(256) for _ in range(32))
    set_id, control_root, control_id = r32(), r32(), (int.from_bytes(r32(), 'big') % m.R).to_bytes(32, 'big')
    vk, td = m.trapdoor_vk(rng, 6)
    sel = b'\x5e\x71\xbe\x0c'
    inner = sm.KeyedRisc0Verifier(vk, sel, control_root, control_id)

    def prove(root):
        sig = inner.signals(m.receipt_claim_ok_digest(set_id, sm.root_journal(set_id, root)))
        return sel + m.proof_to_words(*m.trapdoor_prove(rng, td, sig, 'risc0')), sig
    return dict(rng=rng, r32=r32, set_id=set_id, control_root=control_root, control_id=control_id, vk_words=m.vk_to_words(vk), sel=sel, prove=prove)


class Batch:
    """One device-resident batch; inputs as numpy arrays, uploaded once."""
    def __init__(self, torch, v, ids, jds, blob, off, idx, seals):
        dev = torch.device('cuda', 0)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.torch, self.v, self.n, self.m, self.n_sib = torch, v, len(idx), len(seals) // 260, int(off[-1])
        self.t = [up(ids), up(jds), up(blob), up(off.astype(np.uint32).view(np.int32)), up(idx.astype(np.uint32).view(np.int32)),
                  up(np.concatenate([seals, np.zeros(4, np.uint8)]))]
        self.st = torch.full((self.n,), 255, dtype=torch.uint8, device=dev)
        self.rv = torch.zeros((self.n, 4), dtype=torch.uint8, device=dev)
        self.stream = torch.cuda.Stream()
        torch.cuda.synchronize()

    def __call__(self):
        t = self.t
        self.v.verify_batch_dev(self.n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), self.n_sib, t[4].data_ptr(), self.m,
                                t[5].data_ptr(), self.st.data_ptr(), self.rv.data_ptr(), self.stream.cuda_stream)


def case_hash(torch, args):
    import stylus_zkvm_verifiers_amd as zkv
    n, depth = 1 << args.log2n, args.depth
    g = np.random.default_rng(0x5E71)
    v = zkv.RiscZeroSetInclusionVerifier(bytes(32), bytes(32), bytes(range(32)))
    ids, jds = g.integers(0, 256, 32 * n, dtype=np.uint8), g.integers(0, 256, 32 * n, dtype=np.uint8)
    blob = g.integers(0, 256, 32 * n * depth, dtype=np.uint8)
    b = Batch(torch, v, ids, jds, blob, np.arange(n + 1, dtype=np.uint64) * depth, np.full(n, STORED, dtype=np.uint64), np.zeros(0, np.uint8))
    call_ms = _events(torch, b, b.stream, args.steps)
    hash_ms = _stage_ms(v)[0]
    for _ in range(args.steps):
        b(); b.stream.synchronize()
        hash_ms = min(hash_ms, _stage_ms(v)[0])
    assert (b.st.cpu().numpy() == 1).all() and v.last_counts() == (n, 0, n)
    roofs = _issue_roofs()
    valu = (depth + 1) * 24 * VALU_PER_ROUND + 4 * VALU_PER_SHA
    rate = valu * n / (hash_ms * 1e-3)
    read = n * (64 + 32 * depth + 8 + 4)
    v.close()
    return dict(case='hash', log2n=args.log2n, depth=depth, call_ms=call_ms, k_setincl_hash_ms=hash_ms, claims_per_s=n / (call_ms * 1e-3),
                permutations_per_s=n * (depth + 1) / (hash_ms * 1e-3), valu_lane_instr_per_claim=valu, valu_lane_instr_per_s=rate,
                issue_roofs_lane_instr_per_s=roofs, frac_of_v_mad_u64_u32_roof=rate / roofs['v_mad_u64_u32'], frac_of_v_add_u32_roof=rate / roofs['v_add_u32'],
                bytes_read=read, read_GB_per_s=read / (hash_ms * 1e-3) / 1e9, frac_of_8TB_per_s=read / (hash_ms * 1e-3) / 8e12,
                library=os.path.basename(os.environ.get('ZKV_LIB_PATH', 'libzkv_mi355x.so')))


def _keyed_verifier(td):
    import stylus_zkvm_verifiers_amd as zkv
    return zkv.RiscZeroSetInclusionVerifier(td['control_root'], td['control_id'], td['set_id'], vk_words=td['vk_words'], root_selector=td['sel'])


def _groth16_alone(torch, td, proofs, signals, steps):
    """zkv_groth16_verify_batch_dev on the given proofs (n x 256) and signals (n x 160) alone -> (ms, verdicts)."""
    import stylus_zkvm_verifiers_amd as zkv
    dev = torch.device('cuda', 0)
    g = zkv.Groth16Verifier(td['vk_words'], 6, zkv.errors.VM_RISC0)
    n = len(proofs) // 256
    p, s = torch.from_numpy(proofs.copy()).to(dev), torch.from_numpy(signals.copy()).to(dev)
    out = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    ms = _events(torch, lambda: g.verify_batch_dev(n, p.data_ptr(), s.data_ptr(), out.data_ptr(), stream.cuda_stream), stream, steps)
    res = out.cpu().numpy()
    g.close()
    return ms, res


def case_honest(torch, args):
    import set_inclusion_model as sm
    import spec_model as m
    td = _trapdoor(0xB16)
    n, depth, trees, leaves = 1 << args.log2n, args.depth, 16, 64
    assert depth >= 6
    rows_id, rows_jd, rows_path, rows_idx, seals, proofs, sigs = [], [], [], [], [], [], []
    for t in range(trees):
        ids = [(td['r32'](), td['r32']()) for _ in range(leaves)]
        small, paths = sm.tree_paths([sm.leaf(m.receipt_claim_ok_digest(i, j)) for i, j in ids])
        upper = [td['r32']() for _ in range(depth - 6)]
        root = small
        for s in upper:
            root = sm.node(root, s)
        seal, sig = td['prove'](root)
        seals.append(seal); proofs.append(seal[4:]); sigs.append(b''.join(m.be32(x) for x in sig))
        for (i, j), p in zip(ids, paths):
            rows_id.append(i); rows_jd.append(j); rows_path.append(b''.join(p + upper)); rows_idx.append(t)
    pool = len(rows_idx)
    rep = n // pool
    tile = lambda rows, w: np.tile(np.frombuffer(b''.join(rows), np.uint8).reshape(pool, w), (rep, 1)).reshape(-1)
    v = _keyed_verifier(td)
    b = Batch(torch, v, tile(rows_id, 32), tile(rows_jd, 32), tile(rows_path, 32 * depth), np.arange(pool * rep + 1, dtype=np.uint64) * depth,
              np.tile(np.array(rows_idx, dtype=np.uint64), rep), np.frombuffer(b''.join(seals), np.uint8))
    call_ms = _events(torch, b, b.stream, args.steps)
    stage = _stage_ms(v)
    assert not b.st.cpu().numpy().any() and v.last_counts() == (pool * rep, trees, 0)
    alone_ms, res = _groth16_alone(torch, td, np.frombuffer(b''.join(proofs), np.uint8), np.frombuffer(b''.join(sigs), np.uint8), args.steps)
    assert (res == 1).all()
    v.close()
    return dict(case='honest', log2n=args.log2n, depth=depth, root_seals=trees, call_ms=call_ms, k_setincl_hash_ms=stage[0], groth16_16_proofs_alone_ms=alone_ms,
                feature_cost_ms=call_ms - alone_ms, claims_per_s=pool * rep / (call_ms * 1e-3))


def case_worst(torch, args):
    import spec_model as m
    td = _trapdoor(0x3057)
    n, depth = 1 << 14, args.depth
    g = np.random.default_rng(0x3057)
    seal, sig = td['prove'](td['r32']())
    v = _keyed_verifier(td)
    b = Batch(torch, v, g.integers(0, 256, 32 * n, dtype=np.uint8), g.integers(0, 256, 32 * n, dtype=np.uint8), g.integers(0, 256, 32 * n * depth, dtype=np.uint8),
              np.arange(n + 1, dtype=np.uint64) * depth, np.zeros(n, dtype=np.uint64), np.frombuffer(seal, np.uint8))
    call_ms = _events(torch, b, b.stream, args.steps)
    stage = _stage_ms(v)
    assert (b.st.cpu().numpy() == 1).all() and v.last_counts() == (n, n, 0)
    # the inner call alone: the same proof 2^14 times, every row with other claim-digest halves (what the straggler jobs carry)
    sigs = np.tile(np.frombuffer(b''.join(m.be32(x) for x in sig), np.uint8), (n, 1))
    sigs[:, 80:96] = g.integers(0, 256, (n, 16), dtype=np.uint8); sigs[:, 112:128] = g.integers(0, 256, (n, 16), dtype=np.uint8)
    alone_ms, res = _groth16_alone(torch, td, np.tile(np.frombuffer(seal[4:], np.uint8), n), sigs.reshape(-1), args.steps)
    assert not res.any()
    v.close()
    return dict(case='worst', log2n=14, depth=depth, jobs=n, call_ms=call_ms, k_setincl_hash_ms=stage[0], inner_stage_ms_1_to_4=stage[1:],
                groth16_2p14_proofs_alone_ms=alone_ms, ratio=call_ms / alone_ms)


def case_resources(args):
    from stylus_zkvm_verifiers_amd import build
    keep = ('VGPRs', 'AGPRs', 'TotalSGPRs', 'ScratchSize [bytes/lane]', 'Occupancy [waves/SIMD]', 'LDS Size [bytes/block]')
    rows = [r for r in build.resource_report() if 'setincl' in r['kernel']]
    path = os.path.join(ROOT, 'profiles', 'set_inclusion_resources.txt')
    with open(path, 'w') as f:
        f.write('kernel resources of csrc/k_setincl.hip as hipcc reports them (-Rpass-analysis=kernel-resource-usage, gfx950)\n')
        for r in rows:
            f.write('%s: %s\n' % (r['kernel'], ', '.join('%s %s' % (k, r.get(k)) for k in keep)))
    return dict(case='resources', kernels=len(rows), file=os.path.relpath(path, ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='hash,honest,worst,resources')
    ap.add_argument('--log2n', type=int, default=20)
    ap.add_argument('--depth', type=int, default=20)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'set_inclusion_bench.jsonl'))
    args = ap.parse_args()
    cases = args.cases.split(',')
    torch = None
    if set(cases) - {'resources'}:
        import torch
    for c in cases:
        line = case_resources(args) if c == 'resources' else {'hash': case_hash, 'honest': case_honest, 'worst': case_worst}[c](torch, args)
        print(json.dumps(line))
        with open(args.out, 'a') as f:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
