"""Numpy model of the mixed-batch partition with a per-proof method (csrc/k_mixed.hip, include/zkv.h "mixed batches with a per-proof
method"): which proofs reach which verifier, in which compact order, with which RISC Zero method, and what the unplaced proofs get."""
import numpy as np

STATUS_BAD_CALLDATA, STATUS_UNKNOWN_VM = 6, 7


def classify(vm, method=None):
    """0 = RISC Zero (verify or verify_integrity), 1 = SP1 (verify_proof), 2 = unknown tag, 3 = a method the proof's VM does not have."""
    vm = np.asarray(vm, dtype=np.uint8)
    m = np.zeros_like(vm) if method is None else np.asarray(method, dtype=np.uint8)
    c = np.full(vm.shape, 2, dtype=np.int8)
    c[(vm == 0) & (m <= 1)] = 0
    c[(vm == 0) & (m > 1)] = 3
    c[(vm == 1) & (m == 0)] = 1
    c[(vm == 1) & (m != 0)] = 3
    return c


def partition(vm, method=None):
    """Returns (idx: compact order -> proof index, RISC Zero rows first then SP1, both stable; n0 = RISC Zero rows; kind[n0]: the
    RISC Zero method of each compact row; unplaced: proof indices without a slot; their status bytes (UNKNOWN_VM / BAD_CALLDATA))."""
    c = classify(vm, method)
    m = np.zeros(len(c), dtype=np.uint8) if method is None else np.asarray(method, dtype=np.uint8)
    i0, i1 = np.nonzero(c == 0)[0], np.nonzero(c == 1)[0]
    unplaced = np.nonzero(c >= 2)[0]
    st = np.where(c[unplaced] == 2, STATUS_UNKNOWN_VM, STATUS_BAD_CALLDATA).astype(np.uint8)
    return np.concatenate([i0, i1]), len(i0), m[i0].copy(), unplaced, st


def random_calls(rng, n, p_bad=0.03):
    """About a third each of RISC Zero verify, RISC Zero verify_integrity and SP1 verify_proof, plus a few unknown tags and invalid
    method bytes."""
    kind = rng.integers(0, 3, n)
    vm = np.where(kind == 2, 1, 0).astype(np.uint8)
    method = np.where(kind == 1, 1, 0).astype(np.uint8)
    bad = rng.random(n) < p_bad
    vm[bad & (rng.random(n) < 0.5)] = 2
    method[bad & (vm != 2)] = rng.integers(2, 256, int((bad & (vm != 2)).sum())).astype(np.uint8)
    sp1_bad = (vm == 1) & (rng.random(n) < p_bad / 2)
    method[sp1_bad] = 1                                   # SP1 has no verify_integrity
    return vm, method
