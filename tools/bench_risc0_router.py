"""Throughput of the RISC Zero verifier router (include/zkv_risc0_router.h).

    python tools/bench_risc0_router.py [--cases one,four] [--log2n 16] [--steps 3] [--out FILE]

One JSON line per case (appended to --out, default profiles/risc0_router_bench.jsonl); device-resident batches (torch tensors), best of
--steps timed calls after a warm-up call, every status checked.
  one    2^log2n re-randomised copies of the real RISC Zero proof through a router whose only route is the built-in route with the
         proof's parameters, against zkv_risc0_verify_batch_dev on the same seals: the price of the partition in front of the verifier
  four   four keyed routes (trapdoor keys with n_ic = 6), 2^log2n shuffled seals in one call, against
         (i) zkv_groth16_set_verify_batch_dev on the same proofs with host-prepared signals and key indices -- the nearest existing
             path; it does no selector or digest work -- and
         (ii) four one-route routers on the pre-sorted quarters, summed
Seals: one proof per key re-randomised into 4,096 distinct ones (synth.make_batch / make_groth16_batch), tiled.  Not bench.py.
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

H = bytes.fromhex
POOL = 4096


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(torch.device('cuda', 0))


def status_buffer(n):
    import torch
    return torch.full((n,), 255, dtype=torch.uint8, device=torch.device('cuda', 0))


def timed(fn, steps):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(round((time.perf_counter() - t) * 1e3, 3))
    return out


class RouterCall:
    """One device-resident verify batch on one router."""

    def __init__(self, rt, seals, ids, jds):
        import torch
        self.rt, self.n = rt, len(seals)
        self.d = [up(seals), up(ids), up(jds)]
        self.st = status_buffer(self.n)
        self.s = torch.cuda.current_stream().cuda_stream
        rt.reserve(self.n)

    def __call__(self):
        d = self.d
        self.rt.verify_batch_dev(self.n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), self.st.data_ptr(), 0, self.s)

    def accepted(self):
        return int((self.st.cpu().numpy() == 0).sum())


def trapdoor_pool(seed):
    """(key words, control root, control id, selector, POOL x 260 seals, image id, journal digest, the five signals) of a fresh trapdoor key."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import risc0_router_model as rm
    key = rm.Key(seed)
    rng = random.Random(seed ^ 0x5EED)
    iid = bytes(rng.randrange(256) for _ in range(32)); jd = bytes(rng.randrange(256) for _ in range(32))
    sig = key.route.verifier.signals(m.receipt_claim_ok_digest(iid, jd))
    base = key.prove(iid, jd)[4:]
    p, _, _, _ = synth.make_groth16_batch(key.words, 'risc0', base, sig, POOL, seed=seed, mutate_every=1 << 30)
    seals = np.concatenate([np.tile(np.frombuffer(key.selector, np.uint8), (POOL, 1)), p], axis=1)
    return key, seals, np.frombuffer(iid, np.uint8), np.frombuffer(jd, np.uint8), np.frombuffer(b''.join(m.be32(s) for s in sig), np.uint8)


def case_one(a):
    import torch
    n = 1 << a.log2n
    g = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'real_proofs.json')))['risc0']
    pool, _, _, _ = synth.make_batch('risc0', H(g['seal']), POOL, 0x17D0, mutate_every=0)
    S = np.tile(pool, (n // POOL, 1))
    I, J = np.tile(np.frombuffer(H(g['image_id']), np.uint8), (n, 1)), np.tile(np.frombuffer(H(g['journal_digest']), np.uint8), (n, 1))
    router = RouterCall(zkv.RiscZeroRouter([(H(g['control_root']), H(g['bn254_control_id']))]), S, I, J)
    v = zkv.RiscZeroVerifier(); v.initialize(H(g['control_root']), H(g['bn254_control_id']))
    d = [up(S), up(I), up(J)]
    st = status_buffer(n)
    s = torch.cuda.current_stream().cuda_stream
    zkv._lib.check(v._L.zkv_ctx_reserve(v._h, n), 'zkv_ctx_reserve')

    def direct():
        zkv._lib.check(v._L.zkv_risc0_verify_batch_dev(v._h, n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), st.data_ptr(), None, s), 'zkv_risc0_verify_batch_dev')
    # the verifier set the built-in group is, with the instance row supplied by the caller: what the router's front end adds to
    vs = zkv.RiscZeroVerifierSet([H(g['control_root'])], [H(g['bn254_control_id'])])
    d_inst = up(np.zeros(n, dtype=np.uint32))
    st2 = status_buffer(n)
    zkv._lib.check(vs._L.zkv_ctx_reserve(vs._h, n), 'zkv_ctx_reserve')

    def as_set():
        zkv._lib.check(vs._L.zkv_risc0_set_verify_batch_dev(vs._h, n, d_inst.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), st2.data_ptr(), None, s),
                       'zkv_risc0_set_verify_batch_dev')
    t_r, t_d, t_v = timed(router, a.steps), timed(direct, a.steps), timed(as_set, a.steps)
    ok = router.accepted() == n and int((st.cpu().numpy() == 0).sum()) == n and int((st2.cpu().numpy() == 0).sum()) == n

    def stage(h):
        import ctypes as C
        out = (C.c_float * 5)()
        zkv._lib.check(h._L.zkv_ctx_last_stage_ms(h._h, out), 'zkv_ctx_last_stage_ms')
        return [round(x, 3) for x in out]
    row = dict(case='one_builtin_route', n=n, router_ms=min(t_r), direct_ms=min(t_d), ratio=round(min(t_r) / min(t_d), 4), verifier_set_ms=min(t_v),
               ratio_to_verifier_set=round(min(t_r) / min(t_v), 4), router_all_ms=t_r, direct_all_ms=t_d, verifier_set_all_ms=t_v,
               router_stage_ms=stage(router.rt), direct_stage_ms=stage(v), verifier_set_stage_ms=stage(vs), gt_window_bits=os.environ.get('ZKV_GT_WINDOW_BITS', ''),
               route_counts=router.rt.last_route_counts(), all_accepted=ok)
    router.rt.close(); v.close(); vs.close()
    return row


def case_four(a):
    import torch
    n = 1 << a.log2n
    per = n // 4
    pools = [trapdoor_pool(0x17D10 + k) for k in range(4)]
    S = np.concatenate([np.tile(p[1], (per // POOL, 1)) for p in pools])
    I = np.concatenate([np.tile(p[2], (per, 1)) for p in pools])
    J = np.concatenate([np.tile(p[3], (per, 1)) for p in pools])
    G = np.concatenate([np.tile(p[4], (per, 1)) for p in pools])
    K = np.repeat(np.arange(4, dtype=np.uint32), per)
    perm = np.random.default_rng(0x17D1).permutation(n)
    shared = RouterCall(zkv.RiscZeroRouter(keyed=[p[0].triple() for p in pools]), S[perm], I[perm], J[perm])
    t_s = timed(shared, a.steps)
    ok = shared.accepted() == n
    counts = shared.rt.last_route_counts()
    stage = [round(x, 3) for x in shared.rt.last_stage_ms()]
    shared.rt.close()
    # (i) the key set on the same proofs: key indices and the five signals prepared on the host
    gs = zkv.Groth16VerifierSet([(p[0].words, 6, zkv.errors.VM_RISC0) for p in pools])
    d = [up(K[perm]), up(S[perm][:, 4:]), up(G[perm])]
    ver = status_buffer(n)
    s = torch.cuda.current_stream().cuda_stream
    zkv._lib.check(gs._L.zkv_ctx_reserve(gs._h, n), 'zkv_ctx_reserve')
    t_g = timed(lambda: gs.verify_batch_dev(n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), ver.data_ptr(), s), a.steps)
    ok = ok and int((ver.cpu().numpy() == 1).sum()) == n
    gs.close()
    # (ii) four one-route routers on the pre-sorted quarters
    each = []
    for k, p in enumerate(pools):
        c = RouterCall(zkv.RiscZeroRouter(keyed=[p[0].triple()]), S[per * k:per * (k + 1)], I[per * k:per * (k + 1)], J[per * k:per * (k + 1)])
        each.append(min(timed(c, a.steps)))
        ok = ok and c.accepted() == per
        c.rt.close()
    return dict(case='four_keyed_routes_shuffled', n=n, router_ms=min(t_s), key_set_host_signals_ms=min(t_g), ratio_to_key_set=round(min(t_s) / min(t_g), 4),
                four_one_route_routers_ms=round(sum(each), 3), each_ms=each, ratio_to_four=round(min(t_s) / sum(each), 4), router_all_ms=t_s, key_set_all_ms=t_g,
                router_stage_ms=stage, route_counts=counts, all_accepted=ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='one,four')
    ap.add_argument('--log2n', type=int, default=16)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'risc0_router_bench.jsonl'))
    a = ap.parse_args()
    fns = dict(one=case_one, four=case_four)
    rows = [fns[c](a) for c in a.cases.split(',')]
    with open(a.out, 'a') as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + '\n')
    if not all(r['all_accepted'] for r in rows):
        raise SystemExit('a seal that should verify was rejected')


if __name__ == '__main__':
    main()
