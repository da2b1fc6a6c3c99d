"""Decode and end-to-end time of eth_call batches on the RISC Zero router (include/zkv_risc0_router_wire.h).

    python tools/bench_risc0_router_wire.py [--log2n 16] [--steps 5] [--out FILE]

One JSON line (appended to --out, default profiles/risc0_router_wire_bench.jsonl).  2^log2n `verify` requests over re-randomised copies of
the real RISC Zero proof behind a router whose only route is the built-in route with the proof's parameters; everything device-resident
(torch tensors); one warm-up call per variant, then --steps rounds in which the variants take turns, every status checked:
  router_u   zkv_risc0_router_eth_call_batch_dev, form UINT8_ARRAY calldata (8,452 bytes per request)
  router_b   the same, form BYTES calldata (420 bytes per request)
  decoded    zkv_risc0_router_verify_batch_dev on the same seals, already decoded
  single_u   zkv_eth_call_batch_dev on ONE RISC Zero context with the form UINT8_ARRAY calldata: k_wire_risc0, the kernel k_wire_rzrouter
             was modelled on, in the same session
End-to-end = wall clock around a call that ends in a device synchronise; decode = zkv_ctx_last_wire_ms after it.  Not bench.py.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import stylus_zkvm_verifiers_amd as zkv                 # noqa: E402
from stylus_zkvm_verifiers_amd import synth             # noqa: E402

H = bytes.fromhex
POOL = 4096


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(torch.device('cuda', 0))


def calldata(form, S, iid, jd):
    """n canonical verify calls over the rows of S (n x 260) as one (n x length) array: one encoded request as the template, the seal
    bytes written into every row."""
    n = len(S)
    one = np.frombuffer(zkv.RiscZeroRouter.encode_verify_call(S[0].tobytes(), iid, jd, form=form), dtype=np.uint8)
    cd = np.tile(one, (n, 1))
    if form == 0:
        cd[:, 132 + 31::32] = S
    else:
        cd[:, 132:132 + 260] = S
    assert cd[0].tobytes() == one.tobytes() and cd[-1].tobytes() == zkv.RiscZeroRouter.encode_verify_call(S[-1].tobytes(), iid, jd, form=form)
    return cd


def wire_ms(handle):
    out = C.c_float(0)
    zkv._lib.check(zkv._lib.lib().zkv_ctx_last_wire_ms(handle, C.byref(out)), 'zkv_ctx_last_wire_ms')
    return out.value


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--log2n', type=int, default=16)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'risc0_router_wire_bench.jsonl'))
    a = ap.parse_args()
    n = 1 << a.log2n
    g = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'real_proofs.json')))['risc0']
    iid, jd = H(g['image_id']), H(g['journal_digest'])
    pool, _, _, _ = synth.make_batch('risc0', H(g['seal']), POOL, 0x17D0, mutate_every=0)
    S = np.tile(pool, (max(n // POOL, 1), 1))[:n]
    dev = torch.device('cuda', 0)
    s = torch.cuda.current_stream().cuda_stream
    rt = zkv.RiscZeroRouter([(H(g['control_root']), H(g['bn254_control_id']))])
    rt.reserve(n)
    v = zkv.RiscZeroVerifier(); v.initialize(H(g['control_root']), H(g['bn254_control_id']))
    zkv._lib.check(v._L.zkv_ctx_reserve(v._h, n), 'zkv_ctx_reserve')
    blobs, offs, size = {}, {}, {}
    for form, name in ((0, 'u'), (1, 'b')):
        cd = calldata(form, S, iid, jd)
        size[name] = int(cd.size)
        offs[name] = up((np.arange(n + 1, dtype=np.int64) * cd.shape[1]))
        blobs[name] = up(cd)
        del cd
    d_s, d_i, d_j = up(S), up(np.tile(np.frombuffer(iid, np.uint8), (n, 1))), up(np.tile(np.frombuffer(jd, np.uint8), (n, 1)))
    st = {k: torch.full((n,), 255, dtype=torch.uint8, device=dev) for k in ('router_u', 'router_b', 'decoded', 'single_u')}
    raw = zkv._lib.lib()

    def single_u():
        zkv._lib.check(raw.zkv_eth_call_batch_dev(v._h, n, blobs['u'].data_ptr(), offs['u'].data_ptr(), size['u'], st['single_u'].data_ptr(), None, s),
                       'zkv_eth_call_batch_dev')
    calls = dict(router_u=lambda: rt.eth_call_batch_dev(n, blobs['u'].data_ptr(), offs['u'].data_ptr(), size['u'], st['router_u'].data_ptr(), 0, 0, s),
                 router_b=lambda: rt.eth_call_batch_dev(n, blobs['b'].data_ptr(), offs['b'].data_ptr(), size['b'], st['router_b'].data_ptr(), 0, 0, s),
                 decoded=lambda: rt.verify_batch_dev(n, d_s.data_ptr(), d_i.data_ptr(), d_j.data_ptr(), st['decoded'].data_ptr(), 0, s),
                 single_u=single_u)
    decode_of = dict(router_u=lambda: wire_ms(rt._h), router_b=lambda: wire_ms(rt._h), single_u=lambda: wire_ms(v._h))
    for fn in calls.values():                                # one warm-up each
        fn()
        torch.cuda.synchronize()
    total = {k: [] for k in calls}
    decode = {k: [] for k in decode_of}
    for _ in range(a.steps):                                 # the variants take turns within every round
        for k, fn in calls.items():
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            total[k].append(round((time.perf_counter() - t) * 1e3, 3))
            if k in decode_of:
                decode[k].append(round(decode_of[k](), 4))
    ok = all(int((b.cpu().numpy() == 0).sum()) == n for b in st.values())
    spread = lambda x: round(max(x) / min(x), 4)
    row = dict(bench='risc0_router_wire', n=n, steps=a.steps, calldata_bytes=size,
               total_ms={k: min(x) for k, x in total.items()}, total_all_ms=total, decode_ms={k: min(x) for k, x in decode.items()}, decode_all_ms=decode,
               decode_tb_per_s={k: round(size[k[-1]] / min(x) / 1e9, 3) for k, x in decode.items()},
               decode_u_router_over_single=round(min(decode['router_u']) / min(decode['single_u']), 4),
               decode_round_spread={k: spread(x) for k, x in decode.items()},
               total_over_decoded={k: round(min(total[k]) / min(total['decoded']), 4) for k in ('router_u', 'router_b')},
               total_round_spread={k: spread(x) for k, x in total.items()},
               call_counts=rt.last_call_counts(), all_accepted=ok)
    rt.close(); v.close()
    print(json.dumps(row), flush=True)
    with open(a.out, 'a') as f:
        f.write(json.dumps(row) + '\n')
    if not ok:
        raise SystemExit('a request that should verify was rejected')


if __name__ == '__main__':
    main()
