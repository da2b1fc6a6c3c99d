"""Throughput of the RISC Zero verifier router (include/zkv_risc0_router.h).

    python tools/bench_risc0_router.py [--cases one,four] [--log2n 16] [--steps 3] [--out FILE]
    python tools/bench_risc0_router.py --aggregate [--log2n-aggregate 18] [--steps 3] [--out FILE]

One JSON line per case (appended to --out, default profiles/risc0_router_bench.jsonl); device-resident batches (torch tensors), best of
--steps timed calls after a warm-up call, every status checked.
  one    2^log2n re-randomised copies of the real RISC Zero proof through a router whose only route is the built-in route with the
         proof's parameters, against zkv_risc0_verify_batch_dev on the same seals: the price of the partition in front of the verifier
  four   four keyed routes (trapdoor keys with n_ic = 6), 2^log2n shuffled seals in one call, against
         (i) zkv_groth16_set_verify_batch_dev on the same proofs with host-prepared signals and key indices -- the nearest existing
             path; it does no selector or digest work -- and
         (ii) four one-route routers on the pre-sorted quarters, summed
  --aggregate   the aggregate check on the keyed group (default --out profiles/keyed_group_aggregate_bench.jsonl):
         four keyed routes, 2^log2n-aggregate shuffled seals, check off then on (automatic size) in one process, all seals valid and
         with one seal in 64 damaged (four fifths refused before the pairing, a fifth at it); beside it the same keys and proofs through
         zkv_groth16_set_verify_batch_dev off and on, whose ratio is the yardstick.  Damaged batches are a loss at 2^18, as on sets
         (DESIGN.md section 11a): the second pass costs a kernel latency per stage that this size cannot hide.
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


def trapdoor_pool(seed, mutate_every=1 << 30):
    """(key, POOL x 260 seals, image id, journal digest, the five signals) of a fresh trapdoor key; every mutate_every-th seal has C off the
    curve or B outside the subgroup."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import risc0_router_model as rm
    key = rm.Key(seed)
    rng = random.Random(seed ^ 0x5EED)
    iid = bytes(rng.randrange(256) for _ in range(32)); jd = bytes(rng.randrange(256) for _ in range(32))
    sig = key.route.verifier.signals(m.receipt_claim_ok_digest(iid, jd))
    base = key.prove(iid, jd)[4:]
    p, _, _, _ = synth.make_groth16_batch(key.words, 'risc0', base, sig, POOL, seed=seed, mutate_every=mutate_every, classes=('c_off_curve', 'b_out_of_subgroup'))
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


def case_aggregate(a, damaged):
    import torch
    n = 1 << a.log2n_aggregate
    per = n // 4
    pools = [trapdoor_pool(0x17D10 + k, 64 if damaged else 1 << 30) for k in range(4)]
    S = np.concatenate([np.tile(p[1], (per // POOL, 1)) for p in pools])
    I = np.concatenate([np.tile(p[2], (per, 1)) for p in pools])
    J = np.concatenate([np.tile(p[3], (per, 1)) for p in pools])
    G = np.concatenate([np.tile(p[4], (per, 1)) for p in pools])
    K = np.repeat(np.arange(4, dtype=np.uint32), per)
    bad = n // 64 if damaged else 0
    if damaged:                                                   # a fifth of the damaged seals fail at the pairing instead: a valid seal, other inputs
        at = np.arange(63, n, 64)[::5]
        S[at] = S[at - 1]
        J[at, 31] ^= 1
        G[at, 3 * 32 + 31] ^= 1                                   # (the key set takes signals: any other claim digest half)
    perm = np.random.default_rng(0x17D2).permutation(n)
    call = RouterCall(zkv.RiscZeroRouter(keyed=[p[0].triple() for p in pools]), S[perm], I[perm], J[perm])
    t_off = timed(call, a.steps)
    acc_off, stage_off = call.accepted(), [round(x, 3) for x in call.rt.last_stage_ms()]
    call.rt.set_aggregate_check(True)
    t_on = timed(call, a.steps)
    acc_on, stage_on = call.accepted(), [round(x, 3) for x in call.rt.last_stage_ms()]
    counters = [int(x) for x in call.rt.aggregate_counters()]
    call.rt.close()
    gs = zkv.Groth16VerifierSet([(p[0].words, 6, zkv.errors.VM_RISC0) for p in pools])
    d = [up(K[perm]), up(S[perm][:, 4:]), up(G[perm])]
    ver = status_buffer(n)
    s = torch.cuda.current_stream().cuda_stream
    gs.reserve(n)
    run = lambda: gs.verify_batch_dev(n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), ver.data_ptr(), s)
    g_off = timed(run, a.steps)
    gacc_off, gstage_off = int((ver.cpu().numpy() == 1).sum()), [round(x, 3) for x in gs.last_stage_ms()]
    gs.set_aggregate_check(True)
    g_on = timed(run, a.steps)
    gacc_on, gstage_on = int((ver.cpu().numpy() == 1).sum()), [round(x, 3) for x in gs.last_stage_ms()]
    gs.close()
    ratio, gratio = min(t_on) / min(t_off), min(g_on) / min(g_off)
    return dict(case='aggregate_four_keyed_routes', front_end='risc0_router', n=n, damaged_one_in=64 if damaged else 0, off_ms=min(t_off), on_ms=min(t_on),
                ratio=round(ratio, 4), key_set_off_ms=min(g_off), key_set_on_ms=min(g_on), key_set_ratio=round(gratio, 4), gap=round(ratio / gratio, 4),
                off_all_ms=t_off, on_all_ms=t_on, key_set_off_all_ms=g_off, key_set_on_all_ms=g_on, stage_off_ms=stage_off, stage_on_ms=stage_on,
                key_set_stage_off_ms=gstage_off, key_set_stage_on_ms=gstage_on, aggregate_counters=counters,
                all_accepted=acc_off == acc_on == gacc_off == gacc_on == n - bad and counters[0] > 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='one,four')
    ap.add_argument('--log2n', type=int, default=16)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--aggregate', action='store_true')
    ap.add_argument('--log2n-aggregate', type=int, default=18)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, 'profiles', 'keyed_group_aggregate_bench.jsonl' if a.aggregate else 'risc0_router_bench.jsonl')
    fns = dict(one=case_one, four=case_four)
    rows = [case_aggregate(a, False), case_aggregate(a, True)] if a.aggregate else [fns[c](a) for c in a.cases.split(',')]
    with open(a.out, 'a') as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + '\n')
    if not all(r['all_accepted'] for r in rows):
        raise SystemExit('a seal that should verify was rejected')


if __name__ == '__main__':
    main()
