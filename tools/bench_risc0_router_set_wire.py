"""Measurements of eth_call batches on a RISC Zero router with a set route (include/zkv_risc0_router_set_wire.h).

    python tools/bench_risc0_router_set_wire.py [--cases set,plain,resources] [--log2n 16] [--depth 20] [--rounds 5] [--out FILE]

One JSON line per case (appended to --out, default profiles/risc0_router_set_wire_bench.jsonl); device-resident batches (torch tensors).
The protocol of tools/bench_risc0_router_set.py: one session, the variants of a case take turns, one warm-up call each, then --rounds
rounds; the result is the best round with the spread, every round is recorded (HIP events around the call on its stream; the decode time
is zkv_ctx_last_wire_ms of the same call), every status and count is checked.
  set        2^log2n set-inclusion seals at --depth over 16 distinct valid root seals of one keyed route (bench_risc0_router_set.py's
             `decode` batch), on a router with that keyed route and the set route:
             U  zkv_risc0_router_eth_call_ragged_dev, verify(uint8[],bytes32,bytes32) calldata;
             B  the same entry point, verify(bytes,bytes32,bytes32) calldata;
             R  zkv_risc0_router_verify_ragged_dev on the same decoded seals.
  plain      2^log2n Groth16 requests (one valid seal of a keyed route) on a router without a set route, in both forms: the new entry
             point against zkv_risc0_router_eth_call_batch_dev.  The old entry point's form U decode is k_wire_rzrouter on
             tools/bench_risc0_router_wire.py's form U batch: its rate, in the same session, is the yardstick of the `set` case's.
  resources  VGPRs, scratch, LDS and occupancy of the new and changed kernels from the build logs ->
             profiles/risc0_router_set_wire_resources.txt (no GPU needed)
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


def _take_turns(torch, variants, stream, rounds):
    """Every variant once as a warm-up, then `rounds` rounds in turn -> per variant ([ms end to end], [ms decode or None])."""
    for v in variants:
        v()
    stream.synchronize()
    out = [([], []) for _ in variants]
    for _ in range(rounds):
        for k, v in enumerate(variants):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); v(); e1.record(stream); e1.synchronize()
            out[k][0].append(round(e0.elapsed_time(e1), 4))
            out[k][1].append(round(v.rt.last_wire_ms(), 4) if v.wire else None)
    return out


def _summary(ms):
    return dict(best_ms=min(ms), worst_ms=max(ms), spread_ms=round(max(ms) - min(ms), 4), all_ms=ms)


def _decode_summary(ms, calldata_bytes):
    s = _summary(ms)
    s['TB_per_s_best'] = round(calldata_bytes / (s['best_ms'] * 1e-3) / 1e12, 3)
    s['TB_per_s_worst'] = round(calldata_bytes / (s['worst_ms'] * 1e-3) / 1e12, 3)
    return s


def _word(v):
    return np.frombuffer(int(v).to_bytes(32, 'big'), np.uint8)


def calldata_rows(form, seals, ids, jds):
    """verify(seal, image id, journal digest) of every row in `form`, seals of one length: a (rows, bytes per request) uint8 array."""
    import risc0_router_wire_model as wm
    rows, L = seals.shape
    body = 32 * L if form == wm.FORM_U else wm.pad32(L)
    out = np.zeros((rows, 132 + body), dtype=np.uint8)
    out[:, :4] = np.frombuffer(wm.selector(form, wm.VERIFY), np.uint8)
    out[:, 4:36] = _word(0x60); out[:, 36:68] = ids; out[:, 68:100] = jds; out[:, 100:132] = _word(L)
    if form == wm.FORM_U:
        out[:, 132 + 31::32] = seals
    else:
        out[:, 132:132 + L] = seals
    return out


class Call:
    """One device-resident entry point on uploaded buffers; statuses pre-filled with 255."""

    def __init__(self, torch, rt, fn, wire, arrays, n, stream):
        dev = torch.device('cuda', 0)
        self.rt, self.fn, self.wire, self.n, self.stream = rt, fn, wire, n, stream
        self.t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in arrays]
        self.st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
        self.rv = torch.full((n, 4), 255, dtype=torch.uint8, device=dev)

    def __call__(self):
        self.fn(self)

    def ok(self):
        return not self.st.cpu().numpy().any()


def _eth_call(new):
    def fn(c):
        from stylus_zkvm_verifiers_amd import risc0_router_set_wire as sw, risc0_router_wire as w
        f = sw.eth_call_ragged_dev if new else w.eth_call_batch_dev
        f(c.rt._h, c.n, c.t[0].data_ptr(), c.t[1].data_ptr(), c.t[0].numel(), c.st.data_ptr(), c.rv.data_ptr(), 0, c.stream.cuda_stream)
    return fn


def _ragged(c):
    c.rt.verify_ragged_dev(c.n, c.t[0].data_ptr(), c.t[1].data_ptr(), c.t[0].numel(), c.t[2].data_ptr(), c.t[3].data_ptr(), c.st.data_ptr(), c.rv.data_ptr(),
                           c.stream.cuda_stream)


def _offsets(n, stride):
    return (np.arange(n + 1, dtype=np.uint64) * stride).view(np.int64)


def case_set(torch, args):
    import risc0_router_model as rm
    import risc0_router_wire_model as wm
    import set_inclusion_model as sm
    import spec_model as m
    import stylus_zkvm_verifiers_amd as zkv
    rng = random.Random(0xB17C)
    r32 = lambda: bytes(rng.randrange(256) for _ in range(32))
    key, set_id = rm.Key(0xB17C), m.sha256(b'bench_risc0_router_set_wire')
    n, depth, trees, leaves = 1 << args.log2n, args.depth, 16, 64
    assert depth >= 6 and n % (trees * leaves) == 0
    set_sel = sm.set_selector(set_id)
    rows_id, rows_jd, rows_seal = [], [], []
    for t in range(trees):
        ids = [(r32(), r32()) for _ in range(leaves)]
        small, paths = sm.tree_paths([sm.leaf(m.receipt_claim_ok_digest(i, j)) for i, j in ids])
        upper = [r32() for _ in range(depth - 6)]
        root = small
        for s in upper:
            root = sm.node(root, s)
        seal = key.prove(set_id, sm.root_journal(set_id, root))
        for (i, j), p in zip(ids, paths):
            rows_id.append(i); rows_jd.append(j); rows_seal.append(set_sel + sm.abi_encode_seal(p + upper, seal))
    pool = len(rows_seal)
    rep = n // pool
    arr = lambda rows: np.frombuffer(b''.join(rows), np.uint8).reshape(pool, -1)
    seals, ids, jds = arr(rows_seal), arr(rows_id), arr(rows_jd)
    tile = lambda a: np.tile(a, (rep, 1)).reshape(-1)
    stream = torch.cuda.Stream()
    rt = zkv.RiscZeroSetRouter(set_id, keyed=[key.triple()])
    calls, sizes = [], {}
    for name, form in (('U', wm.FORM_U), ('B', wm.FORM_B)):
        cd = calldata_rows(form, seals, ids, jds)
        sizes[name] = n * cd.shape[1]
        calls.append(Call(torch, rt, _eth_call(True), True, [tile(cd), _offsets(n, cd.shape[1])], n, stream))
    calls.append(Call(torch, rt, _ragged, False, [tile(seals), _offsets(n, seals.shape[1]), tile(ids), tile(jds)], n, stream))
    torch.cuda.synchronize()
    res = _take_turns(torch, calls, stream, args.rounds)
    counts = []
    for c in calls:                                                  # the counts of each variant's own call
        c(); stream.synchronize()
        counts.append((rt.set_last_counts(), rt.last_call_counts()))
    ok = all(c.ok() for c in calls) and all(k == ((n, trees, trees, 0), [0, n, 0, 0, 0]) for k in counts)
    row = dict(case='set', log2n=args.log2n, depth=depth, root_seals=trees, seal_bytes=int(seals.shape[1]), calldata_GB={k: round(v / 1e9, 3) for k, v in sizes.items()},
               eth_call_form_u=_summary(res[0][0]), eth_call_form_b=_summary(res[1][0]), verify_ragged=_summary(res[2][0]),
               decode_form_u=_decode_summary(res[0][1], sizes['U']), decode_form_b=_decode_summary(res[1][1], sizes['B']),
               ratio_u=round(min(res[0][0]) / min(res[2][0]), 4), ratio_b=round(min(res[1][0]) / min(res[2][0]), 4), all_as_expected=bool(ok))
    rt.close()
    return row


def case_plain(torch, args):
    import risc0_router_model as rm
    import risc0_router_wire_model as wm
    import stylus_zkvm_verifiers_amd as zkv
    rng = random.Random(0xB17D)
    r32 = lambda: bytes(rng.randrange(256) for _ in range(32))
    key = rm.Key(0xB17D)
    n = 1 << args.log2n
    a, b = r32(), r32()
    one = lambda v: np.frombuffer(v, np.uint8).reshape(1, -1)
    stream = torch.cuda.Stream()
    rt = zkv.RiscZeroRouter(keyed=[key.triple()])
    rt.reserve(n)
    calls, sizes = [], {}
    for name, form in (('U', wm.FORM_U), ('B', wm.FORM_B)):
        cd = calldata_rows(form, one(key.prove(a, b)), one(a), one(b))
        assert wm.decode(cd[0].tobytes()) is not None
        sizes[name] = n * cd.shape[1]
        for new in (True, False):
            calls.append(Call(torch, rt, _eth_call(new), True, [np.tile(cd, (n, 1)).reshape(-1), _offsets(n, cd.shape[1])], n, stream))
    torch.cuda.synchronize()
    res = _take_turns(torch, calls, stream, args.rounds)
    ok = all(c.ok() for c in calls) and rt.last_call_counts() == [n, 0, 0, 0]
    row = dict(case='plain', log2n=args.log2n, calldata_GB={k: round(v / 1e9, 3) for k, v in sizes.items()},
               form_u_new=_summary(res[0][0]), form_u_old=_summary(res[1][0]), form_b_new=_summary(res[2][0]), form_b_old=_summary(res[3][0]),
               decode_form_u_new=_decode_summary(res[0][1], sizes['U']), decode_form_u_old_k_wire_rzrouter=_decode_summary(res[1][1], sizes['U']),
               decode_form_b_new=_decode_summary(res[2][1], sizes['B']), decode_form_b_old=_decode_summary(res[3][1], sizes['B']), all_as_expected=bool(ok))
    rt.close()
    return row


def case_resources(args):
    from stylus_zkvm_verifiers_amd import build
    keep = ('VGPRs', 'AGPRs', 'TotalSGPRs', 'ScratchSize [bytes/lane]', 'Occupancy [waves/SIMD]', 'LDS Size [bytes/block]')
    rows = [r for r in build.resource_report() if 'rzset' in r['kernel'] or 'k_wire_rzrouter' in r['kernel']]
    path = os.path.join(ROOT, 'profiles', 'risc0_router_set_wire_resources.txt')
    with open(path, 'w') as f:
        f.write('kernel resources of csrc/k_wire_rzset.hip (new) and csrc/k_rzrouter_set.hip (k_rzset_front and k_rzset_hash changed) as hipcc reports them\n'
                '(-Rpass-analysis=kernel-resource-usage, gfx950), with k_wire_rzrouter of csrc/k_wire.hip (unchanged) beside them\n')
        for r in rows:
            f.write('%s: %s\n' % (r['kernel'], ', '.join('%s %s' % (k, r.get(k)) for k in keep)))
    return dict(case='resources', kernels=len(rows), file=os.path.relpath(path, ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='set,plain,resources')
    ap.add_argument('--log2n', type=int, default=16)
    ap.add_argument('--depth', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'risc0_router_set_wire_bench.jsonl'))
    args = ap.parse_args()
    cases = args.cases.split(',')
    torch = None
    if set(cases) - {'resources'}:
        import torch
    bad = False
    for c in cases:
        line = case_resources(args) if c == 'resources' else {'set': case_set, 'plain': case_plain}[c](torch, args)
        print(json.dumps(line), flush=True)
        with open(args.out, 'a') as f:
            f.write(json.dumps(line) + '\n')
        bad = bad or line.get('all_as_expected') is False
    if bad:
        raise SystemExit('a status or a count is not what the case expects')


if __name__ == '__main__':
    main()
