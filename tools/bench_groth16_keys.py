"""Throughput of generic Groth16 keys by key length (include/zkv.h "Groth16 core, arbitrary verification key"; DESIGN.md "Long keys").

    python tools/bench_groth16_keys.py [--n-ic 2,6,7,17,33,65,129] [--log2n 16,18] [--steps 3] [--forced 2,6]

Per (n_ic, batch) one JSON line: proofs/s of device-resident batches (zkv_groth16_verify_batch_dev, best of --steps timed calls after a
warm-up call), zkv_ctx_last_stage_ms of the last call, and for the long-key path the vk_x stage's share of the measured issue roof
(zkv_diag_issue_rate, v_mad_u64_u32): multiply-adds of the walk counted on the host (tests/host_sim/host_sim_long_key.cpp, one lane per
proof, as stage_mul_counts.json counts the other stages) over the stage time.  --forced lists keys with n_ic <= 6 that run a second time
with ZKV_LONG_KEY=1 (read at context creation), for the A/B against the default path.  Proofs: one trapdoor proof re-randomised into 4,096
distinct ones (synth.make_groth16_batch), tiled on the device; every proof must verify.  Not bench.py: this is a tool of its own.
"""
import argparse
import ctypes as C
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))


def host_mads(vkb, n_ic, sig_bytes):
    """multiply-adds of one proof's long-key walk (None when the host build is unavailable)."""
    src = os.path.join(ROOT, 'tests', 'host_sim', 'host_sim_long_key.cpp')
    lib = os.path.join(ROOT, 'tests', 'host_sim', 'libhost_sim_long_key.so')
    try:
        if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
            subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-Wno-unknown-pragmas', '-o', lib, src], timeout=600)
        L = C.CDLL(lib)
    except (OSError, subprocess.SubprocessError):
        return None
    L.hsl_msm_mads.argtypes = [C.c_char_p, C.c_int, C.c_char_p]
    L.hsl_msm_mads.restype = C.c_ulonglong
    return int(L.hsl_msm_mads(vkb, n_ic, b''.join(sig_bytes) + b'\0'))


def issue_roof():
    from stylus_zkvm_verifiers_amd import _lib
    L = _lib.lib()
    best = 0.0
    for w in (2, 4, 8):
        r = C.c_double(0)
        _lib.check(L.zkv_diag_issue_rate(0, 0, w, 2000, C.byref(r), None), 'zkv_diag_issue_rate')
        best = max(best, r.value)
    return best


def run(n_ic, log2n, steps, forced, roof):
    import torch
    import spec_model as m
    import stylus_zkvm_verifiers_amd as zkv
    from stylus_zkvm_verifiers_amd import synth
    rng = random.Random(n_ic)
    vk, td = m.trapdoor_vk(rng, n_ic)
    vkb = m.vk_to_words(vk)
    sig = [rng.randrange(m.R) for _ in range(n_ic - 1)]
    base = m.proof_to_words(*m.trapdoor_prove(rng, td, sig, 'sp1'))
    proofs, sigs, _, _ = synth.make_groth16_batch(vkb, 'sp1', base, sig, 4096, seed=n_ic, mutate_every=0)
    dev = torch.device('cuda', 0)
    p0 = torch.from_numpy(proofs).to(dev)
    s0 = torch.from_numpy(sigs.reshape(4096, -1).copy()).to(dev)
    mads = host_mads(vkb, n_ic, [m.be32(s) for s in sig]) if (n_ic > 6 or forced) else None
    out = []
    for lg in log2n:
        n = 1 << lg
        reps = n // 4096
        d_p = p0.repeat(reps, 1).contiguous()
        d_s = s0.repeat(reps, 1).contiguous()
        d_v = torch.zeros(n, dtype=torch.uint8, device=dev)
        if forced:
            os.environ['ZKV_LONG_KEY'] = '1'
        v = zkv.Groth16Verifier(vkb, n_ic, zkv.errors.VM_SP1)
        os.environ.pop('ZKV_LONG_KEY', None)
        v.reserve(n)
        sp = d_s.data_ptr() if n_ic > 1 else 0
        v.verify_batch_dev(n, d_p.data_ptr(), sp, d_v.data_ptr())
        v.synchronize()
        ok = int(d_v.sum().item()) == n
        best = None
        for _ in range(steps):
            t0 = time.perf_counter()
            v.verify_batch_dev(n, d_p.data_ptr(), sp, d_v.data_ptr())
            v.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        st = v.last_stage_ms()
        rec = {'n_ic': n_ic, 'proofs': n, 'long_key_path': n_ic > 6 or forced, 'forced_long_key': forced, 'all_verified': ok,
               'proofs_per_s': n / best, 'batch_ms': best * 1e3, 'last_stage_ms': st}
        if mads is not None:
            # the last chunk's stage [1] stands for every chunk of the batch (chunks are equal but the last may be shorter)
            chunk = 64
            while chunk < (1 << 20) and 2 * chunk * 32 * (n_ic - 1) <= (1 << 29):
                chunk *= 2
            chunk = min(n, chunk)
            rec.update({'msm_mads_per_proof': mads, 'msm_chunk_proofs': chunk, 'issue_roof_mad_per_s': roof,
                        'msm_share_of_issue_roof': (mads * chunk / (st[1] * 1e-3)) / roof if st[1] > 0 and roof else None})
        print(json.dumps(rec), flush=True)
        out.append(rec)
        v.close()
        del d_p, d_s, d_v
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-ic', default='2,6,7,17,33,65,129')
    ap.add_argument('--log2n', default='16,18')
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--forced', default='6', help='keys with n_ic <= 6 to run again through the long-key path (ZKV_LONG_KEY=1)')
    a = ap.parse_args()
    if a.steps < 1:
        ap.error('--steps must be at least 1')
    log2n = [int(x) for x in a.log2n.split(',') if x]
    if any(x < 12 for x in log2n):
        ap.error('batches start at 2^12 proofs (4,096 distinct proofs are tiled)')
    roof = issue_roof()
    for n_ic in [int(x) for x in a.n_ic.split(',') if x]:
        run(n_ic, log2n, a.steps, False, roof)
        if n_ic <= 6 and str(n_ic) in a.forced.split(','):
            run(n_ic, log2n, a.steps, True, roof)


if __name__ == '__main__':
    main()
