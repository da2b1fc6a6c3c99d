"""eth_call batches on the SP1 gateway (include/zkv_sp1_gateway_wire.h) against the entry points that take decoded input.

    python tools/bench_sp1_gateway_wire.py [--log2n 16] [--steps 5] [--out FILE]

One JSON line per case (appended to --out, default profiles/sp1_gateway_wire_bench.jsonl); everything device-resident (torch tensors), one
warm-up call per variant, then --steps rounds in which the variants of a case alternate; best of the rounds, all rounds kept.  Times are a
host clock around a call that ends in a device synchronise; decode_ms is zkv_ctx_last_wire_ms (device events around k_wire_gateway).
  mixed    2^log2n requests, 3/4 SP1 Groth16 and 1/4 SP1 PLONK in random order, to a gateway (Groth16 route + one PLONK route): form U
           calldata, form B calldata, and zkv_sp1_gateway_verify_batch_dev on the same proofs already decoded
  groth16  2^log2n SP1 Groth16 requests in form U: the gateway against zkv_eth_call_batch_dev on an SP1 context (and form B, and decoded)
Every status of every variant is checked against the decoded-input call.  Proofs as tools/bench_sp1_gateway.py.  Not bench.py.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import stylus_zkvm_verifiers_amd as zkv                 # noqa: E402
from stylus_zkvm_verifiers_amd import synth, wire       # noqa: E402
from bench_sp1_gateway import pools                      # noqa: E402


def calldata(form, blob, off, vkeys, pvs, kind):
    """Canonical calls of one form for a synth.make_sp1_gateway_batch batch: (blob uint8[], offsets uint64[n + 1])."""
    n = len(kind)
    rows = {}
    for k in (0, 1):
        idx = np.nonzero(kind == k)[0]
        if not len(idx):
            continue
        plen, vlen = int(off[idx[0] + 1] - off[idx[0]]), pvs.shape[1]
        tmpl = np.frombuffer(zkv.Sp1Gateway.encode_verify_proof_call(bytes(32), bytes(vlen), bytes(plen), form=form), np.uint8)
        span = (lambda L: 32 * L) if form == 0 else (lambda L: (L + 31) // 32 * 32)
        pv_at, proof_at = 132, 132 + span(vlen) + 32
        R = np.tile(tmpl, (len(idx), 1))
        R[:, 4:36] = vkeys[idx]
        P = np.stack([blob[int(off[i]):int(off[i]) + plen] for i in idx])
        if form == 0:
            R[:, pv_at + 31:pv_at + 32 * vlen:32] = pvs[idx]
            R[:, proof_at + 31:proof_at + 32 * plen:32] = P
        else:
            R[:, pv_at:pv_at + vlen] = pvs[idx]
            R[:, proof_at:proof_at + plen] = P
        rows[k] = (R, iter(range(len(idx))))
    lens = np.array([rows[int(k)][0].shape[1] for k in kind], dtype=np.uint64)
    coff = np.zeros(n + 1, dtype=np.uint64); coff[1:] = np.cumsum(lens)
    out = np.empty(int(coff[-1]), dtype=np.uint8)
    for i in range(n):
        R, it = rows[int(kind[i])]
        out[int(coff[i]):int(coff[i + 1])] = R[next(it)]
    return out, coff


def case(name, n, frac, gp, pp, key, steps):
    import torch
    dev = torch.device('cuda', 0)
    s = torch.cuda.current_stream().cuda_stream
    blob, off, vkeys, pvs, kind, _, _ = synth.make_sp1_gateway_batch(gp, pp, n, frac, 0x6A7EC + n)
    gw = zkv.Sp1Gateway(True, [key])
    sp1 = zkv.Sp1Verifier() if frac == 1.0 else None
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev)
    d_vk, d_pv, d_p, d_off = up(vkeys), up(pvs), up(blob), up(off.view(np.int64))
    cd = {}
    for form, tag in ((0, 'form_u'), (1, 'form_b')):
        b, o = calldata(form, blob, off, vkeys, pvs, kind)
        cd[tag] = (up(b), up(o.view(np.int64)), len(b))
    outs = {}

    def out(tag):
        if tag not in outs:
            outs[tag] = (torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(4 * n, dtype=torch.uint8, device=dev))
        return outs[tag]

    def run_decoded():
        st, rv = out('decoded')
        gw.verify_batch_dev(n, d_vk.data_ptr(), d_pv.data_ptr(), pvs.shape[1], d_p.data_ptr(), d_off.data_ptr(), len(blob), st.data_ptr(), rv.data_ptr(), s)

    def run_form(tag):
        def f():
            st, rv = out(tag)
            gw.eth_call_batch_dev(n, cd[tag][0].data_ptr(), cd[tag][1].data_ptr(), cd[tag][2], st.data_ptr(), rv.data_ptr(), s)
        return f

    def run_sp1():
        st, rv = out('sp1_ctx_form_u')
        wire.eth_call_batch_dev(sp1, n, cd['form_u'][0].data_ptr(), cd['form_u'][1].data_ptr(), cd['form_u'][2], st.data_ptr(), rv.data_ptr(), s)

    variants = [('decoded', run_decoded), ('form_u', run_form('form_u')), ('form_b', run_form('form_b'))]
    if sp1 is not None:
        variants.append(('sp1_ctx_form_u', run_sp1))
    gw.reserve(n)
    if sp1 is not None:
        sp1.reserve(n)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    for _, fn in variants:
        timed(fn)
    times = {tag: [] for tag, _ in variants}
    decode = {}
    for _ in range(steps):
        for tag, fn in variants:
            times[tag].append(timed(fn))
            if tag.startswith('form_'):
                decode.setdefault(tag, []).append(gw.last_wire_ms())
            elif tag == 'sp1_ctx_form_u':
                decode.setdefault(tag, []).append(wire.last_wire_ms(sp1))
    want = out('decoded')[0].cpu().numpy()
    equal = {tag: bool((out(tag)[0].cpu().numpy() == want).all()) for tag, _ in variants}
    best = {tag: min(v) for tag, v in times.items()}
    row = dict(case=name, n=n, groth16=int((kind == 0).sum()), plonk=int((kind == 1).sum()), accepted=int((want == 0).sum()),
               calldata_mb={tag: round(cd[tag][2] / 1e6, 1) for tag in cd}, ms={tag: round(v, 3) for tag, v in best.items()},
               decode_ms={tag: round(min(v), 3) for tag, v in decode.items()},
               decode_gb_per_s={tag: round(cd['form_u' if tag != 'form_b' else 'form_b'][2] / min(v) / 1e6, 1) for tag, v in decode.items()},
               over_decoded_ms={tag: round(v - best['decoded'], 3) for tag, v in best.items() if tag.startswith('form_')},
               all_ms={tag: [round(x, 3) for x in v] for tag, v in times.items()}, statuses_equal=equal, call_counts=gw.last_call_counts())
    gw.close()
    if sp1 is not None:
        sp1.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='mixed,groth16')
    ap.add_argument('--log2n', type=int, default=16)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sp1_gateway_wire_bench.jsonl'))
    a = ap.parse_args()
    gp, pp, key = pools()
    rows = []
    for c in a.cases.split(','):
        if c == 'mixed':
            rows.append(case('mixed_3g_1p', 1 << a.log2n, 0.75, gp, pp, key, a.steps))
        elif c == 'groth16':
            rows.append(case('all_groth16', 1 << a.log2n, 1.0, gp, pp, key, a.steps))
        else:
            raise SystemExit('unknown case %r' % c)
    with open(a.out, 'a') as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + '\n')
    if not all(all(r['statuses_equal'].values()) for r in rows):
        raise SystemExit('statuses through calldata differ from the decoded-input call')


if __name__ == '__main__':
    main()
