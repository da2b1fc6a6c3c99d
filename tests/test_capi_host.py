"""C ABI on a machine without a GPU: the library loads, exports every symbol include/zkv.h declares, the host-side
context logic (initialize / selector / VK digest / revert bytes) matches the golden vectors, and compute entry points
fail loudly (ZKV_ERR_NO_DEVICE) instead of falling back to a CPU path."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = bytes.fromhex


@pytest.fixture(scope='module')
def z():
    from stylus_zkvm_verifiers_amd import build
    build.build(verbose=False)
    import stylus_zkvm_verifiers_amd as pkg
    return pkg


def test_every_declared_symbol_is_exported(z):
    from stylus_zkvm_verifiers_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'zkv.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(zkv_[a-z0-9_]+)\s*\(', hdr))
    assert len(declared) >= 25
    L = C.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(L, name), 'missing export: ' + name
    assert declared == set(_lib.SYMBOLS), (declared ^ set(_lib.SYMBOLS))


def test_risc0_context_host_logic(z, real_proofs):
    r = real_proofs['risc0']
    v = z.RiscZeroVerifier()
    assert not v.is_initialized()
    assert v.get_selector() == b'\0' * 4
    v.initialize(H(r['control_root']), H(r['bn254_control_id']))
    assert v.is_initialized()
    assert v.get_selector().hex() == r['selector']
    assert tuple(x.hex() for x in v.get_control_root()) == (r['control_root_0'], r['control_root_1'])
    assert v.get_bn254_control_id().hex() == r['bn254_control_id']
    assert v.get_verifier_key_digest().hex() == r['vk_digest']
    with pytest.raises(z.VerifierError) as ei:
        v.initialize(H(r['control_root']), H(r['bn254_control_id']))
    assert ei.value.status == z.errors.STATUS_ALREADY_INITIALIZED
    assert ei.value.revert.hex() == '0dc149f0'


def test_sp1_constants(z, real_proofs):
    s = z.Sp1Verifier()
    assert s.version() == real_proofs['sp1']['version'] == 'v5.0.0'
    assert s.verifier_hash().hex() == real_proofs['sp1']['verifier_hash']
    assert s.verifier_hash()[:4].hex() == real_proofs['sp1']['selector']


def test_revert_bytes(z, revert_vectors):
    for c in revert_vectors:
        vm = 0 if c['vm'] == 'risc0' else 1
        assert z.errors.revert_bytes(vm, c['status'], H(c['received']), H(c['expected'])).hex() == c['revert']


def test_uninitialised_verifier_needs_no_device(z, real_proofs):
    """risc0/verifier.rs:84-86: the initialisation gate comes before everything else."""
    r = real_proofs['risc0']
    v = z.RiscZeroVerifier()
    st, rv = v.verify_batch([H(r['seal'])] * 3, [H(r['image_id'])] * 3, [H(r['journal_digest'])] * 3)
    assert list(st) == [2, 2, 2]
    with pytest.raises(z.VerifierError) as ei:
        v.verify(H(r['seal']), H(r['image_id']), H(r['journal_digest']))
    assert ei.value.status == 2 and ei.value.revert.hex() == 'f92ee8a9'


def test_no_cpu_fallback(z, real_proofs):
    if z.device_count() > 0:
        pytest.skip('a gfx950 device is present')
    from stylus_zkvm_verifiers_amd import _lib
    r = real_proofs['risc0']
    v = z.RiscZeroVerifier(); v.initialize(H(r['control_root']), H(r['bn254_control_id']))
    with pytest.raises(_lib.ZkvRuntimeError) as ei:
        v.verify(H(r['seal']), H(r['image_id']), H(r['journal_digest']))
    assert ei.value.code == _lib.ERR_NO_DEVICE
    s = real_proofs['sp1']
    with pytest.raises(_lib.ZkvRuntimeError):
        z.Sp1Verifier().verify_proof(H(s['vkey']), H(s['public_values']), H(s['proof']))


def test_argument_validation(z):
    from stylus_zkvm_verifiers_amd import _lib
    L = _lib.lib()
    assert L.zkv_host_register(None, 16) == _lib.ERR_INVALID_ARG and L.zkv_host_unregister(None) == _lib.ERR_INVALID_ARG
    if z.device_count() == 0:
        out = C.c_uint64(7)
        assert L.zkv_diag_wait_faults(0, C.byref(out)) == _lib.ERR_NO_DEVICE and out.value == 0
    if z.device_count() == 0:                   # pinning is a device-runtime service: no device, no silent success
        buf = C.create_string_buffer(4096)
        assert L.zkv_host_register(C.addressof(buf), 4096) == _lib.ERR_NO_DEVICE
    assert L.zkv_risc0_get_selector(None, C.create_string_buffer(4)) == _lib.ERR_WRONG_CTX
    sp = z.Sp1Verifier()
    assert L.zkv_risc0_get_selector(sp._h, C.create_string_buffer(4)) == _lib.ERR_WRONG_CTX
    assert L.zkv_status_abi_encode(7, 1, b'\0' * 4, b'\0' * 4, C.create_string_buffer(68)) == _lib.ERR_INVALID_ARG


def test_wire_layer_host_side(z, wire_cases):
    """Function selectors and the calldata encoders run on the host: they must reproduce the golden calldata bytes."""
    from wire_util import calldata_of
    import oracle_lib as ol
    for sig, sel in wire_cases['selectors'].items():
        assert z.wire.function_selector(sig).hex() == sel
    for c in wire_cases['cases']:
        cd = calldata_of(c, z.wire.encode_risc0_verify, z.wire.encode_risc0_verify_integrity, z.wire.encode_sp1_verify_proof)
        assert ol.keccak256(cd).hex() == c['calldata_keccak'], c['name']
    if z.device_count() == 0:            # no device: eth_call batches fail loudly as well
        from stylus_zkvm_verifiers_amd import _lib
        with pytest.raises(_lib.ZkvRuntimeError) as ei:
            z.wire.eth_call_batch(z.Sp1Verifier(), [z.wire.function_selector('version()')])
        assert ei.value.code == _lib.ERR_NO_DEVICE


def test_bench_fails_loudly_without_a_gpu(z):
    """bench.py must not fall back to a CPU path: without a HIP device it exits with an explicit message."""
    import subprocess
    import sys
    if z.device_count() > 0:
        pytest.skip('a gfx950 device is present')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '1', '--warmup', '0'], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert 'no HIP device' in (p.stderr + p.stdout)
    assert '"metric"' not in p.stdout


def test_bench_output_dump_stays_in_budget(tmp_path):
    """bench.py --dump-outputs: status bytes as float32, whole below 64 MB; a batch too large for it is a fixed seeded sample whose
    index file names the rows, the same from run to run."""
    import sys
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    for n, world in ((1 << 20, 1), (1 << 25, 1), (1 << 24, 8)):
        st = torch.from_numpy((np.arange(n) % 7).astype(np.uint8))
        for run in ('a', 'b'):
            d = tmp_path / ('%d_%d_%s' % (n, world, run))
            for r in range(world):
                bench.dump_outputs(str(d), [st], r, world)
            assert sum(f.stat().st_size for f in d.iterdir()) <= bench.DUMP_BYTES
        sfx = '_rank%d' % (world - 1) if world > 1 else ''
        a = np.load(d / ('status%s.npy' % sfx))
        assert a.dtype == np.float32
        if n * 4 <= bench.DUMP_BYTES // 2 // world:
            assert (a == np.arange(n) % 7).all()
        else:
            i = np.load(d / ('status_index%s.npy' % sfx))
            assert i.dtype == np.float64 and (a == i % 7).all()
            assert (np.load(tmp_path / ('%d_%d_a' % (n, world)) / ('status_index%s.npy' % sfx)) == i).all()


def test_bench_rejects_zero_steps():
    """--steps sets the number of timed steps; ms_per_step is the time of one, so a run without a timed step is an error."""
    import subprocess
    import sys
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and '--steps' in p.stderr


def test_offsets_running_backwards_are_rejected(z, real_proofs):
    """Caller-supplied offsets index the blob inside the kernels: non-monotonic offsets are an argument error, not a read."""
    import numpy as np
    from stylus_zkvm_verifiers_amd import _lib
    L = _lib.lib()
    r = real_proofs['risc0']
    v = z.RiscZeroVerifier(); v.initialize(H(r['control_root']), H(r['bn254_control_id']))
    blob = H(r['seal']) * 2 + b'\0'
    bad = np.array([0, 520, 260], dtype=np.uint64)
    ids = H(r['image_id']) * 2; jds = H(r['journal_digest']) * 2
    st = np.zeros(2, dtype=np.uint8)
    assert L.zkv_risc0_verify_batch(v._h, 2, blob, bad.ctypes.data, ids, jds, st.ctypes.data, None) == _lib.ERR_INVALID_ARG
    rev = np.zeros(2, dtype=np.uint8); ret = np.zeros(2 * 96, dtype=np.uint8); rl = np.zeros(2, dtype=np.uint32)
    assert L.zkv_risc0_eth_call_batch(v._h, 2, blob, bad.ctypes.data, rev.ctypes.data, ret.ctypes.data, rl.ctypes.data, None) == _lib.ERR_INVALID_ARG
    sp = z.Sp1Verifier()
    good = np.array([0, 260, 520], dtype=np.uint64)
    assert L.zkv_sp1_verify_batch(sp._h, 2, ids, blob, bad.ctypes.data, blob, good.ctypes.data, st.ctypes.data, None) == _lib.ERR_INVALID_ARG


def test_hot_kernels_keep_their_resources(z):
    """What the compiler reported for the library that was just loaded (build/*.log, hipcc -Rpass-analysis=kernel-resource-usage): the two
    kernels that carry 96 % of a batch have no scratch frame, no spilled VGPR, two wavefronts per SIMD and their LDS budget.  (Round 2 removed
    45.8 + 69.9 GB of scratch traffic per 2^20-proof launch from them; this keeps it out.)"""
    from stylus_zkvm_verifiers_amd import build
    rep = {r['kernel']: r for r in build.resource_report()}
    hot = {k: v for k, v in rep.items() if 'k_miller2' in k or 'k_finalexp2' in k}
    if len(hot) < 2:
        pytest.skip('no build logs next to the library (prebuilt .so only)')
    for name, r in hot.items():
        assert int(r['ScratchSize [bytes/lane]']) == 0 and int(r['VGPRs Spill']) == 0, (name, r)
        assert int(r['Occupancy [waves/SIMD]']) >= 2 and int(r['AGPRs']) == 0, (name, r)
        assert int(r['LDS Size [bytes/block]']) <= 18432, (name, r)
    # round 4: the vk_x stage keeps no private copy of the scalars any more (432 bytes of scratch per lane until then)
    for name, r in rep.items():
        if 'k_msmE' in name or 'k_vk_x' in name:
            assert int(r['ScratchSize [bytes/lane]']) == 0 and int(r['VGPRs Spill']) == 0, (name, r)
    # the small-batch kernels of round 3: the two-wavefront Miller kernels keep everything in registers and LDS, and none of the
    # kernels of that translation unit may push the inversion they share into AGPRs (that cost k_finalexp_w its second wavefront once)
    small = {k: v for k, v in rep.items() if 'w64' in k or 'k_miller_w' in k or 'k_finalexp_w' in k}
    assert len(small) >= 6, sorted(small)
    for name, r in small.items():
        assert int(r['Occupancy [waves/SIMD]']) >= 2 and int(r['AGPRs']) == 0, (name, r)
        if 'w64d' in name:
            assert int(r['ScratchSize [bytes/lane]']) == 0 and int(r['LDS Size [bytes/block]']) <= 20480, (name, r)
    # the shared-accumulator Miller kernels (aggregate check, ecPairing seam): the running points live in HBM rows so that LDS holds f only
    shared = {k: v for k, v in rep.items() if 'k_agg_miller' in k or 'k_pairing_miller_g' in k}
    assert len(shared) >= 6, sorted(shared)
    for name, r in shared.items():
        assert int(r['ScratchSize [bytes/lane]']) == 0 and int(r['VGPRs Spill']) == 0 and int(r['AGPRs']) == 0, (name, r)
        assert int(r['Occupancy [waves/SIMD]']) >= 2 and int(r['LDS Size [bytes/block]']) <= 12288, (name, r)


def test_chunk_capacity_is_clamped(z):
    """ZKV_CHUNK is clamped to [64, 2^26]: the lane-pair kernels address a chunk's workspace rows through 32-bit lane offsets
    ((8 * cap + i) * 4 bytes in k_miller2), which wrap from cap = 2^32 / 36 on.  Read per call, in a fresh process each."""
    import subprocess
    import sys
    code = 'from stylus_zkvm_verifiers_amd import _lib; print(_lib.lib().zkv_chunk_capacity())'
    for env, want in (('', 1 << 20), ('1', 64), ('100', 128), (str(1 << 26), 1 << 26), (str((1 << 26) + 1), 1 << 26), (str(1 << 40), 1 << 26),
                      ('18446744073709551615', 1 << 26)):
        e = dict(os.environ, PYTHONPATH=ROOT)
        e.pop('ZKV_CHUNK', None)
        if env:
            e['ZKV_CHUNK'] = env
        out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=e, timeout=300)
        assert out.returncode == 0, out.stderr
        got = int(out.stdout.strip().splitlines()[-1])
        assert got == want, (env, got, want)
        assert (8 * got + got) * 4 < 1 << 32                      # the largest lane offset k_miller2 forms


def test_bench_self_launches_its_ranks_and_propagates_failure(z):
    """`python bench.py --gpus 2` with no launcher (no WORLD_SIZE in the environment) starts the two ranks itself, as child processes;
    on a box without a GPU both fail loudly, the failure is propagated as the exit code and nothing that looks like a result is printed."""
    import subprocess
    import sys
    if z.device_count() > 0:
        pytest.skip('a gfx950 device is present')
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '0', '--workload', 'risc0_2p16', '--proofs', '64',
                        '--no-cpu-baseline'], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode != 0
    assert 'no HIP device' in p.stderr
    assert '"metric"' not in p.stdout
    # under a launcher whose WORLD_SIZE disagrees with --gpus the mismatch is an explicit message, not an assertion trace
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '0', '--workload', 'risc0_2p16', '--proofs', '64'],
                       capture_output=True, text=True, timeout=600, env=dict(env, WORLD_SIZE='1', RANK='0'))
    assert p.returncode != 0 and 'launch one process per GPU' in p.stderr


def test_aggregate_check_switch_host_side(z, real_proofs):
    """zkv_ctx_set_aggregate_check touches no device: accepted values (0, 1, 16, 32, 64) on every context kind that has a pairing equation
    of its own, a caller's seed or the operating system's, refused on a precompile context and for other sub-batch sizes; the counters of a
    context that never ran are zero."""
    import ctypes as C
    L = z._lib.lib()
    r = real_proofs['risc0']
    v = z.RiscZeroVerifier(); v.initialize(H(r['control_root']), H(r['bn254_control_id']))
    sp = z.Sp1Verifier()
    mx = z.MixedVerifier(H(r['control_root']), H(r['bn254_control_id']))
    for ctx in (v, sp, mx):
        for en in (1, 16, 32, 64, 128, 256, 0):
            assert L.zkv_ctx_set_aggregate_check(ctx._h, en, None) == 0
            assert L.zkv_ctx_set_aggregate_check(ctx._h, en, bytes(32)) == 0
        for en in (2, 8, 48, 512, -1):
            assert L.zkv_ctx_set_aggregate_check(ctx._h, en, None) != 0
        assert ctx.aggregate_counters() == (0, 0)
    assert L.zkv_ctx_set_aggregate_check(None, 1, None) != 0
    pc = z.Bn254Precompiles()
    assert L.zkv_ctx_set_aggregate_check(pc._h, 1, None) != 0 and L.zkv_ctx_set_aggregate_check(pc._h, 0, None) == 0
    with pytest.raises(ValueError):
        v.set_aggregate_check(True, seed=b'short')
    for ctx in (v, sp, mx, pc):
        ctx.close()


def test_device_memory_count_without_a_device(z, real_proofs):
    """zkv_diag_device_memory needs no device: {0 allocations, 0 bytes} before and after one context of every kind this module creates has
    been created, asked to compute (refused: no device) and destroyed."""
    if z.device_count() > 0:
        pytest.skip('a gfx950 device is present: tests/test_device_memory_gpu.py counts there')
    from stylus_zkvm_verifiers_amd import _lib
    L = _lib.lib()

    def live():
        out = (C.c_uint64 * 2)(7, 7)
        assert L.zkv_diag_device_memory(out) == _lib.OK
        return out[0], out[1]
    assert L.zkv_diag_device_memory(None) == _lib.ERR_INVALID_ARG
    assert live() == (0, 0)
    r = real_proofs['risc0']
    v = z.RiscZeroVerifier(); v.initialize(H(r['control_root']), H(r['bn254_control_id']))
    ctxs = [v, z.Sp1Verifier(), z.MixedVerifier(H(r['control_root']), H(r['bn254_control_id'])), z.Bn254Precompiles()]
    for ctx in ctxs:
        assert L.zkv_ctx_reserve(ctx._h, 64) == _lib.ERR_NO_DEVICE
    assert live() == (0, 0)
    for ctx in ctxs:
        ctx.close()
    assert live() == (0, 0)
