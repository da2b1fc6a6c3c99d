"""Throughput of the SP1 gateway's Groth16 routes with caller-supplied keys (include/zkv_sp1_gateway_keys.h).

    python tools/bench_sp1_gateway_keys.py [--cases one,four,guard] [--log2n 18] [--log2n-guard 20] [--steps 3] [--keyed 1] [--out FILE]
    python tools/bench_sp1_gateway_keys.py --aggregate [--log2n 18] [--steps 3] [--out FILE]

One JSON line per case (appended to --out, default profiles/sp1_gateway_keys_bench.jsonl); device-resident batches (torch tensors), best of
--steps timed calls after a warm-up call, every status checked.
  one    2^log2n re-randomised copies of the real SP1 proof through a gateway whose only route is a keyed route holding the v5.0.0 key and
         hash, against a gateway with the built-in route on the same proofs: the price of a caller key (8-bit long-key rows, no GT tables)
  four   four keyed routes (trapdoor keys), 2^log2n shuffled proofs in one call, against four one-route gateways on the pre-sorted
         sub-batches (summed): what the shared pass is for
  guard  2^log2n-guard proofs, all for the built-in route, on a gateway that has the built-in route and (--keyed 1) two keyed routes none
         of whose proofs appear; --keyed 0 builds the plain gateway (the only one a library without this header has; set ZKV_LIB_PATH to
         measure another build of the library)
  --aggregate   the aggregate check on the keyed group (default --out profiles/keyed_group_aggregate_bench.jsonl):
         four keyed routes, 2^log2n shuffled proofs, check off then on (automatic size) in one process, all proofs valid and with one
         proof in 64 damaged (four fifths refused before the pairing, a fifth at it); beside it the same keys and proofs through
         zkv_groth16_set_verify_batch_dev off and on, whose ratio is the yardstick.  Damaged batches are a loss at 2^18, as on sets
         (DESIGN.md section 11a): the second pass costs a kernel latency per stage that this size cannot hide.
Proofs: one proof per key re-randomised into 4,096 distinct ones (synth.make_batch / make_groth16_batch), tiled.  Not bench.py.
"""
import argparse
import hashlib
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


def real_pool():
    g = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'real_proofs.json')))['sp1']
    seals, _, _, _ = synth.make_batch('sp1', H(g['proof']), POOL, 0x12D0B, mutate_every=0)
    return seals, np.frombuffer(H(g['vkey']), np.uint8), np.frombuffer(H(g['public_values']), np.uint8)


def trapdoor_pool(seed, pv_len, mutate_every=1 << 30):
    """(key words, verifier hash, POOL x 260 proofs, program vkey, public values) of a fresh trapdoor key; every mutate_every-th proof
    has C off the curve or B outside the subgroup."""
    rng = random.Random(seed)
    vk, td = m.trapdoor_vk(rng, 3)
    vkey = int(rng.randrange(m.R)).to_bytes(32, 'big')
    pv = bytes(rng.randrange(256) for _ in range(pv_len))
    sig = [int.from_bytes(vkey, 'big'), m.sp1_hash_public_values(pv)]
    words = m.vk_to_words(vk)
    base = m.proof_to_words(*m.trapdoor_prove(rng, td, sig, 'sp1'))
    p, _, _, _ = synth.make_groth16_batch(words, 'sp1', base, sig, POOL, seed=seed, mutate_every=mutate_every, classes=('c_off_curve', 'b_out_of_subgroup'))
    vh = hashlib.sha256(b'bench keyed route %d' % seed).digest()
    seals = np.concatenate([np.tile(np.frombuffer(vh[:4], np.uint8), (POOL, 1)), p], axis=1)
    return words, vh, seals, np.frombuffer(vkey, np.uint8), np.frombuffer(pv, np.uint8)


class Call:
    """One device-resident batch of fixed-length proofs on one gateway."""

    def __init__(self, gw, seals, vkeys, pvs):
        import torch
        dev = torch.device('cuda', 0)
        self.gw, self.n, self.pv_len = gw, len(seals), pvs.shape[1]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev)
        off = np.arange(self.n + 1, dtype=np.int64) * seals.shape[1]
        self.bytes = int(off[-1])
        self.d = [up(vkeys), up(pvs), up(seals), up(off)]
        self.st = torch.full((self.n,), 255, dtype=torch.uint8, device=dev)
        self.s = torch.cuda.current_stream().cuda_stream
        gw.reserve(self.n)

    def __call__(self):
        d = self.d
        self.gw.verify_batch_dev(self.n, d[0].data_ptr(), d[1].data_ptr(), self.pv_len, d[2].data_ptr(), d[3].data_ptr(), self.bytes, self.st.data_ptr(), 0, self.s)

    def accepted(self):
        return int((self.st.cpu().numpy() == 0).sum())


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


def case_one(a):
    n = 1 << a.log2n
    seals, vkey, pv = real_pool()
    S, V, W = np.tile(seals, (n // POOL, 1)), np.tile(vkey, (n, 1)), np.tile(pv, (n, 1))
    keyed = Call(zkv.Sp1Gateway(False, groth16_keys=[(m.vk_to_words(m.SP1_VK), m.SP1_VERIFIER_HASH)]), S, V, W)
    builtin = Call(zkv.Sp1Gateway(True), S, V, W)
    t_k, t_b = timed(keyed, a.steps), timed(builtin, a.steps)
    ok = keyed.accepted() == n and builtin.accepted() == n
    row = dict(case='one_keyed_route_v5_key', n=n, keyed_ms=min(t_k), builtin_ms=min(t_b), ratio=round(min(t_k) / min(t_b), 4), keyed_all_ms=t_k,
               builtin_all_ms=t_b, keyed_stage_ms=[round(x, 3) for x in keyed.gw.last_stage_ms()],
               builtin_stage_ms=[round(x, 3) for x in builtin.gw.last_stage_ms()], all_accepted=ok)
    keyed.gw.close(); builtin.gw.close()
    return row


def case_four(a):
    n = 1 << a.log2n
    per = n // 4
    pools = [trapdoor_pool(0x12D10 + k, 96) for k in range(4)]
    S = np.concatenate([np.tile(p[2], (per // POOL, 1)) for p in pools])
    V = np.concatenate([np.tile(p[3], (per, 1)) for p in pools])
    W = np.concatenate([np.tile(p[4], (per, 1)) for p in pools])
    perm = np.random.default_rng(0x12D1).permutation(n)
    shared = Call(zkv.Sp1Gateway(False, groth16_keys=[(p[0], p[1]) for p in pools]), S[perm], V[perm], W[perm])
    t_s = timed(shared, a.steps)
    ok = shared.accepted() == n
    counts = shared.gw.last_route_counts()
    stage = [round(x, 3) for x in shared.gw.last_stage_ms()]
    shared.gw.close()
    each = []
    for k, p in enumerate(pools):
        c = Call(zkv.Sp1Gateway(False, groth16_keys=[(p[0], p[1])]), S[per * k:per * (k + 1)], V[per * k:per * (k + 1)], W[per * k:per * (k + 1)])
        each.append(min(timed(c, a.steps)))
        ok = ok and c.accepted() == per
        c.gw.close()
    return dict(case='four_keyed_routes_shuffled', n=n, shared_pass_ms=min(t_s), four_one_route_gateways_ms=round(sum(each), 3), each_ms=each,
                ratio=round(min(t_s) / sum(each), 4), shared_all_ms=t_s, shared_stage_ms=stage, route_counts=counts, all_accepted=ok)


def case_guard(a):
    n = 1 << a.log2n_guard
    seals, vkey, pv = real_pool()
    S, V, W = np.tile(seals, (n // POOL, 1)), np.tile(vkey, (n, 1)), np.tile(pv, (n, 1))
    keys = [trapdoor_pool(0x12D20 + k, 96)[:2] for k in range(2)] if a.keyed else []
    c = Call(zkv.Sp1Gateway(True, groth16_keys=keys), S, V, W)
    t = timed(c, a.steps)
    row = dict(case='guard_all_builtin', n=n, keyed_routes=len(keys), ms=min(t), all_ms=t, mproofs_per_s=round(n / min(t) / 1e3, 4),
               route_counts=c.gw.last_route_counts(), all_accepted=c.accepted() == n, lib=os.environ.get('ZKV_LIB_PATH', ''))
    c.gw.close()
    return row


def case_aggregate(a, damaged):
    import torch
    n = 1 << a.log2n
    per = n // 4
    pools = [trapdoor_pool(0x12D10 + k, 96, 64 if damaged else 1 << 30) for k in range(4)]
    S = np.concatenate([np.tile(p[2], (per // POOL, 1)) for p in pools])
    V = np.concatenate([np.tile(p[3], (per, 1)) for p in pools])
    W = np.concatenate([np.tile(p[4], (per, 1)) for p in pools])
    K = np.repeat(np.arange(4, dtype=np.uint32), per)
    sig = [np.frombuffer(bytes(p[3]) + m.be32(m.sp1_hash_public_values(bytes(p[4]))), np.uint8) for p in pools]
    G = np.concatenate([np.tile(g, (per, 1)) for g in sig])
    bad = n // 64 if damaged else 0
    if damaged:                                                   # a fifth of the damaged proofs fail at the pairing instead: a valid proof, other public values
        at = np.arange(63, n, 64)[::5]
        S[at] = S[at - 1]
        W[at, 95] ^= 1
        G[at, 63] ^= 1                                            # (the key set takes signals: any other hash)
    perm = np.random.default_rng(0x12D2).permutation(n)
    call = Call(zkv.Sp1Gateway(False, groth16_keys=[(p[0], p[1]) for p in pools]), S[perm], V[perm], W[perm])
    t_off = timed(call, a.steps)
    acc_off, stage_off = call.accepted(), [round(x, 3) for x in call.gw.last_stage_ms()]
    call.gw.set_aggregate_check(True)
    t_on = timed(call, a.steps)
    acc_on, stage_on = call.accepted(), [round(x, 3) for x in call.gw.last_stage_ms()]
    counters = [int(x) for x in call.gw.aggregate_counters()]
    call.gw.close()
    gs = zkv.Groth16VerifierSet([(p[0], 3, zkv.errors.VM_SP1) for p in pools])
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to(torch.device('cuda', 0))
    d = [up(K[perm]), up(S[perm][:, 4:]), up(G[perm])]
    ver = torch.full((n,), 255, dtype=torch.uint8, device=torch.device('cuda', 0))
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
    return dict(case='aggregate_four_keyed_routes', front_end='sp1_gateway', n=n, damaged_one_in=64 if damaged else 0, off_ms=min(t_off), on_ms=min(t_on),
                ratio=round(ratio, 4), key_set_off_ms=min(g_off), key_set_on_ms=min(g_on), key_set_ratio=round(gratio, 4), gap=round(ratio / gratio, 4),
                off_all_ms=t_off, on_all_ms=t_on, key_set_off_all_ms=g_off, key_set_on_all_ms=g_on, stage_off_ms=stage_off, stage_on_ms=stage_on,
                key_set_stage_off_ms=gstage_off, key_set_stage_on_ms=gstage_on, aggregate_counters=counters,
                all_accepted=acc_off == acc_on == gacc_off == gacc_on == n - bad and counters[0] > 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='one,four,guard')
    ap.add_argument('--log2n', type=int, default=18)
    ap.add_argument('--log2n-guard', type=int, default=20)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--keyed', type=int, default=1)
    ap.add_argument('--aggregate', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, 'profiles', 'keyed_group_aggregate_bench.jsonl' if a.aggregate else 'sp1_gateway_keys_bench.jsonl')
    fns = dict(one=case_one, four=case_four, guard=case_guard)
    rows = [case_aggregate(a, False), case_aggregate(a, True)] if a.aggregate else [fns[c](a) for c in a.cases.split(',')]
    with open(a.out, 'a') as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + '\n')
    if not all(r['all_accepted'] for r in rows):
        raise SystemExit('a proof that should verify was rejected')


if __name__ == '__main__':
    main()
