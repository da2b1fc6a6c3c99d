"""Known-answer tests of the field, tower, G1 and G2 primitives ON THE DEVICE (zkv_diag_primitive): the code the verify kernels run -- carry
builtins, the non-inlined f2_mul_ni / l9_mul_ni leaves, the DPP exchange inside a lane pair, Fp12 values in LDS, the wide routines with
several cases per wavefront -- at the edges of each primitive's contract, against Python integers and oracle/spec_model.py.  Where the
host build of the same harness (tests/host_sim/host_sim_selftest*.cpp) can be compiled, the device words must also be bit-identical to
the host build's words for the same cases.  Case generators and references: tests/primitive_cases.py."""
import functools
import subprocess

import numpy as np
import pytest

import primitive_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    import stylus_zkvm_verifiers_amd as z
    from stylus_zkvm_verifiers_amd import diag_primitive
    assert z.device_count() >= 1, 'no gfx950 device'
    return diag_primitive.lib()


@functools.lru_cache(maxsize=None)
def _host_available(paired):
    try:
        pc.host_lib(paired)
        return True
    except (OSError, subprocess.CalledProcessError):         # no host compiler: the device results are still checked against Python
        return False


def run(lib, mapping, op, n, same_as_host=None, seed=7):
    """one call with all n cases of the op; checks the results, and the first `same_as_host` (default all) against the host build"""
    return run_cases(lib, mapping, op, pc.cases_for(mapping, op, n, seed), same_as_host)


def run_cases(lib, mapping, op, ins, same_as_host=None):
    n = len(ins)
    out = pc.run_device(lib, mapping, op, ins)
    pc.check(mapping, op, ins, out)
    if _host_available(mapping != 0):
        k = n if same_as_host is None else min(n, same_as_host)
        host = pc.run_host(mapping, op, ins[:k])
        diff = np.nonzero((host != out[:k]).any(axis=1))[0]
        assert len(diff) == 0, 'device and host words differ for cases %s' % list(diff[:8])
    return out


# ---------------------------------------------------------------- one value per lane (k_selftest_lane)
def test_lane_fp_linear_ops(lib):
    run(lib, 0, 0, 64 * 64 + 1)


def test_lane_fp_mul_and_sqr(lib):
    run(lib, 0, 1, 64 * 64 + 1)


def test_lane_fp_from_raw_to_raw(lib):
    run(lib, 0, 2, 64 * 16 + 1)


def test_lane_fp_inv(lib):
    run(lib, 0, 3, 64 * 32 + 1)


def test_lane_fp2_products_and_inverse(lib):
    run(lib, 0, 4, 64 * 48 + 1)


def test_lane_fr_ops(lib):
    run(lib, 0, 5, 64 * 32 + 1)


def test_lane_glv_split(lib):
    run(lib, 0, 6, 64 * 48 + 1)


def test_lane_g1_jacobian_ops(lib):
    run(lib, 0, 7, 64 * 16 + 1)


def test_small_batches_are_padded(lib):
    """1 and 31 cases (the rest of the wavefront, pair block or group runs on zero operands and is discarded)"""
    for mapping, op in ((0, 1), (0, 7), (1, 0), (1, 3), (2, 1), (3, 1), (0, 8), (1, 5), (1, 6), (1, 7), (2, 2), (3, 2),
                        (0, 9), (0, 10), (1, 8), (1, 9), (2, 3), (3, 3)):
        for n in (1, 31) if mapping < 2 else (1, 5):
            run(lib, mapping, op, n, seed=n)
    for mapping, op in ((1, 3), (2, 0), (3, 0), (1, 8)):         # a lone case with every word at 2p - 1 beside the zero padding
        run_cases(lib, mapping, op, pc.all_hot_case(mapping, op))


# ---------------------------------------------------------------- lane pairs (k_selftest_pair)
def test_pair_fp2_ops_through_the_dpp_exchange(lib):
    run(lib, 1, 0, 32 * 64 + 1, same_as_host=512)


def test_pair_l9_lincomb_at_every_call_site(lib):
    run(lib, 1, 1, 32 * 32 + 1)


def test_pair_l9_mul(lib):
    run(lib, 1, 2, 32 * 32 + 1, same_as_host=512)


def test_pair_fp12_routines_in_lds(lib):
    run(lib, 1, 3, 32 * 3 + 1)


def test_pair_cyclotomic_squarings(lib):
    run(lib, 1, 4, 32 * 2 + 1)


# ---------------------------------------------------------------- wide groups (k_selftest_wide_s1 / _s4)
def test_wide_sixteen_lanes_fp12_routines(lib):
    run(lib, 2, 0, 4 * 8 + 1)


def test_wide_sixteen_lanes_cyclotomic_squaring(lib):
    run(lib, 2, 1, 4 * 8 + 1)


def test_wide_one_wavefront_fp12_routines(lib):
    run(lib, 3, 0, 9)


def test_wide_one_wavefront_cyclotomic_squaring(lib):
    run(lib, 3, 1, 9)


# ---------------------------------------------------------------- the accept predicates, one 0 / 1 word per lane
def run_predicates(lib, mapping, op, n):
    """The cases must be able to tell a right predicate from a subtly wrong one (checked on the reference alone, before anything is
    compared); then every lane of a case must return the reference's verdict -- the lane that stores the status in the verify kernels
    (word 0 of each verdict) holds its partner's half only through the DPP exchange, which the host build does not run."""
    pc.assert_predicate_cases_bite(mapping, op, pc.cases_for(mapping, op, n, 7))
    run(lib, mapping, op, n)


def test_lane_fp2_is_zero_and_eq(lib):
    run_predicates(lib, 0, 8, 64 * 8 + 1)


def test_pair_fp2_is_zero_and_eq_in_both_lanes(lib):
    run_predicates(lib, 1, 5, 32 * 12 + 1)


def test_pair_fp12_is_one_and_eq_conj_in_both_lanes(lib):
    run_predicates(lib, 1, 6, 32 * 12 + 1)


def test_pair_miller_point_closes_in_both_lanes(lib):
    run_predicates(lib, 1, 7, 32 * 12 + 1)


def test_wide_sixteen_lanes_is_one_in_every_lane(lib):
    run_predicates(lib, 2, 2, 4 * 24 + 1)


def test_wide_one_wavefront_is_one_in_every_lane(lib):
    run_predicates(lib, 3, 2, 48 + 1)


# ---------------------------------------------------------------- G2: Jacobian group ops, membership, Miller line steps
def run_g2(lib, mapping, op, n):
    """The cases must show every 0 / 1 output, and Z' = 0 of the line steps, in both values often enough and in every place (on the
    reference alone); then the device words against the Python reference and, bit for bit, against the host build."""
    pc.assert_g2_cases_bite(mapping, op, pc.cases_for(mapping, op, n, 7))
    run(lib, mapping, op, n)


def test_lane_g2_jacobian_ops_and_membership(lib):
    run_g2(lib, 0, 9, 64 * 16 + 1)


def test_lane_line_steps_frobenius_and_table_lines(lib):
    run_g2(lib, 0, 10, 64 * 16 + 1)


def test_pair_line_steps_as_the_miller_loop_runs_them(lib):
    run_g2(lib, 1, 8, 32 * 12 + 1)


def test_pair_g2_membership_in_both_lanes(lib):
    run_g2(lib, 1, 9, 32 * 6 + 1)              # every point of the pools; the host build's lane threads are the slow part


def test_wide_sixteen_lanes_line_steps_and_line_products(lib):
    run_g2(lib, 2, 3, 4 * 24 + 1)


def test_wide_one_wavefront_line_steps_and_line_products(lib):
    run_g2(lib, 3, 3, 48 + 1)


# ---------------------------------------------------------------- raw operands at the bounds of the contract
def run_bounds(lib, mapping, op, same_as_host=None):
    """Raw Montgomery words at which the lazy sums of a fused body are largest -- 2p - 1 in every place, hot against cold halves, full
    29-bit limbs -- where the tests above hand the same routines v R mod p, a random-looking word.  The batch must hold every structured
    pattern, and each extreme value in every operand position at both case parities (on the inputs alone); then the device words
    against the Python reference, below 2p, and bit for bit against the host build."""
    ins = pc.bound_cases_for(mapping, op)
    pc.assert_bound_cases_bite(mapping, op, ins)
    run_cases(lib, mapping, op, ins, same_as_host)


def test_pair_fp12_routines_at_raw_operand_bounds(lib):
    run_bounds(lib, 1, 3)


def test_pair_cyclotomic_squarings_at_raw_operand_bounds(lib):
    run_bounds(lib, 1, 4)


def test_wide_sixteen_lanes_fp12_routines_at_raw_operand_bounds(lib):
    run_bounds(lib, 2, 0)


def test_wide_sixteen_lanes_cyclotomic_squaring_at_raw_operand_bounds(lib):
    run_bounds(lib, 2, 1)


def test_wide_one_wavefront_fp12_routines_at_raw_operand_bounds(lib):
    run_bounds(lib, 3, 0)


def test_wide_one_wavefront_cyclotomic_squaring_at_raw_operand_bounds(lib):
    run_bounds(lib, 3, 1)


def test_lane_line_steps_at_raw_operand_bounds(lib):
    run_bounds(lib, 0, 10)


def test_pair_line_steps_at_raw_operand_bounds(lib):
    run_bounds(lib, 1, 8)


def test_wide_sixteen_lanes_line_steps_at_raw_operand_bounds(lib):
    run_bounds(lib, 2, 3)


def test_wide_one_wavefront_line_steps_at_raw_operand_bounds(lib):
    run_bounds(lib, 3, 3)


def test_lane_g1_jacobian_ops_at_raw_z_bounds(lib):
    run_bounds(lib, 0, 7)


def test_lane_g2_jacobian_ops_at_raw_z_bounds(lib):
    run_bounds(lib, 0, 9)
